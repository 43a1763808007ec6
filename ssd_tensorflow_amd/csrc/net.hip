// SSD-VGG step executor for gfx950.  See net.h.
#include "net.h"
#include <cmath>
#include <algorithm>
#include <cstdlib>
#include <atomic>
#include <mutex>

namespace ssd {

static bool first_layer_kernel(const ConvDesc& d) { return d.Ci * d.KH * d.KW <= 32 && d.Co == 64; }

// ---------------------------------------------------------------------------------
// graph (ssdvgg.py:190-372)
// ---------------------------------------------------------------------------------
int Net::add_tensor(const std::string& name, int H, int W, int C, bool relu_out) {
    Tensor t;
    t.name = name; t.H = H; t.W = W; t.C = C; t.relu_out = relu_out;
    tensors_.push_back(t);
    return (int)tensors_.size() - 1;
}

enum PadMode { PAD_SAME, PAD_VALID, PAD_BR1_VALID };

void Net::build_graph() {
    const Preset& p = *preset_;
    const int nv = C_ + 5;
    input_t_ = add_tensor("image_input", p.image_h, p.image_w, 3, false);
    int cur = input_t_;

    auto conv = [&](const std::string& name, int cout, int k, int stride, PadMode pm, int dil, bool relu, int head,
                    int from) -> int {
        const Tensor in = tensors_[from];
        Op op;
        op.kind = OP_CONV; op.name = name; op.in = from; op.KH = op.KW = k; op.stride = stride; op.dil = dil;
        op.relu = relu; op.head = head;
        int Ho, Wo;
        if (pm == PAD_SAME) {
            tf_same(in.H, k, stride, dil, &op.pad_h, &Ho);
            tf_same(in.W, k, stride, dil, &op.pad_w, &Wo);
        } else {
            const int keff = (k - 1) * dil + 1;
            const int extra = pm == PAD_BR1_VALID ? 1 : 0;     // tf.pad bottom/right +1 (ssdvgg.py:328-329)
            op.pad_h = op.pad_w = 0;
            Ho = (in.H + extra - keff) / stride + 1;
            Wo = (in.W + extra - keff) / stride + 1;
        }
        op.out = add_tensor(head >= 0 ? "head" + std::to_string(head) : name, Ho, Wo, cout, relu);
        tensors_[from].consumers++;
        ops_.push_back(op);
        return op.out;
    };
    auto pool = [&](const std::string& name, int k, int stride, int from) -> int {
        const Tensor in = tensors_[from];
        Op op;
        op.kind = OP_POOL; op.name = name; op.in = from; op.k = k; op.stride = stride;
        int Ho, Wo;
        tf_same(in.H, k, stride, 1, &op.pad_h, &Ho);
        tf_same(in.W, k, stride, 1, &op.pad_w, &Wo);
        op.out = add_tensor(name, Ho, Wo, in.C, false);
        tensors_[from].consumers++;
        ops_.push_back(op);
        return op.out;
    };

    // VGG-16 trunk (external SavedModel in the reference; ssdvgg.py:195-207)
    cur = conv("conv1_1", 64, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv1_2", 64, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = pool("pool1", 2, 2, cur);
    cur = conv("conv2_1", 128, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv2_2", 128, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = pool("pool2", 2, 2, cur);
    cur = conv("conv3_1", 256, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv3_2", 256, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv3_3", 256, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = pool("pool3", 2, 2, cur);
    cur = conv("conv4_1", 512, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv4_2", 512, 3, 1, PAD_SAME, 1, true, -1, cur);
    const int c43 = cur = conv("conv4_3", 512, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = pool("pool4", 2, 2, cur);
    cur = conv("conv5_1", 512, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv5_2", 512, 3, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv5_3", 512, 3, 1, PAD_SAME, 1, true, -1, cur);
    // a-trous modifications (ssdvgg.py:231-292), or VGG-16's fully connected layers as convolutions (ssdvgg.py:210-228)
    cur = pool("mod_pool5", 3, 1, cur);
    if (fc_) {
        cur = conv("mod_conv6", 4096, 7, 1, PAD_SAME, 1, true, -1, cur);
    } else {
        cur = conv("mod_conv6", 1024, 3, 1, PAD_SAME, 6, true, -1, cur);
    }
    const int c7 = cur = conv("mod_conv7", fc_ ? 4096 : 1024, 1, 1, PAD_SAME, 1, true, -1, cur);
    // extra feature layers (ssdvgg.py:300-332)
    const bool big = p.nmaps >= 7;
    std::vector<int> fmaps{-1, c7};
    cur = conv("conv8_1", 256, 1, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv8_2", 512, 3, 2, PAD_SAME, 1, true, -1, cur); fmaps.push_back(cur);
    cur = conv("conv9_1", 128, 1, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv9_2", 256, 3, 2, PAD_SAME, 1, true, -1, cur); fmaps.push_back(cur);
    cur = conv("conv10_1", 128, 1, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv10_2", 256, 3, big ? 2 : 1, big ? PAD_SAME : PAD_VALID, 1, true, -1, cur); fmaps.push_back(cur);
    cur = conv("conv11_1", 128, 1, 1, PAD_SAME, 1, true, -1, cur);
    cur = conv("conv11_2", 256, 3, 1, PAD_VALID, 1, true, -1, cur); fmaps.push_back(cur);
    if (big) {
        cur = conv("conv12_1", 128, 1, 1, PAD_SAME, 1, true, -1, cur);
        cur = conv("conv12_2", 256, 3, 1, PAD_BR1_VALID, 1, true, -1, cur); fmaps.push_back(cur);
    }
    // l2 norm on conv4_3 (ssdvgg.py:335-337), then the fused multibox heads (ssdvgg.py:353-365)
    {
        Op op;
        op.kind = OP_L2NORM; op.name = "l2_norm_conv4_3"; op.in = c43;
        op.out = add_tensor("norm_conv4_3", tensors_[c43].H, tensors_[c43].W, tensors_[c43].C, false);
        tensors_[c43].consumers++;
        ops_.push_back(op);
        fmaps[0] = op.out;
    }
    SSD_REQUIRE((int)fmaps.size() == p.nmaps, "feature map count mismatch");
    {
        int hw[MAX_MAPS];
        for (int i = 0; i < p.nmaps; ++i) hw[i] = p.map_size[i] * p.map_size[i];
        heads_ = head_layout(p.nmaps, hw, p.ntypes, nv);
    }
    SSD_REQUIRE(heads_.A == p.num_anchors, "head layout has %d anchors, preset says %d", heads_.A, p.num_anchors);
    for (int i = 0; i < p.nmaps; ++i) {
        SSD_REQUIRE(tensors_[fmaps[i]].H == p.map_size[i], "feature map %d is %d, preset says %d", i, tensors_[fmaps[i]].H,
                    p.map_size[i]);
        SSD_REQUIRE(heads_.off[i] == p.off[i], "head layout: map %d starts at anchor %d, preset says %d", i, heads_.off[i], p.off[i]);
        head_t_.push_back(conv("heads/map" + std::to_string(i), heads_.ld[i], 3, 1, PAD_SAME, 1, false, i, fmaps[i]));
    }
    heads_.grad_bf16 = bf16_ ? 1 : 0;
    if (bf16_) {
        for (size_t i = 0; i < tensors_.size(); ++i) tensors_[i].data_f32 = tensors_[i].grad_f32 = false;
        tensors_[input_t_].data_f32 = true;                 // the image is consumed as fed (fp32)
        for (int t : head_t_) tensors_[t].data_f32 = true;   // the loss reads fp32 logits / offsets
    }

    tail_first_ = (int)ops_.size();
    for (size_t i = 0; i < ops_.size(); ++i)
        if (ops_[i].name == "conv8_1") tail_first_ = (int)i;
    build_orders();
    // ---- arena layout: all filters (forward order), all biases, the l2-norm scale ----
    size_t off = 0;
    for (auto& op : ops_)
        if (op.kind == OP_CONV) {
            op.w_off = off;
            off += (size_t)op.KH * op.KW * tensors_[op.in].C * tensors_[op.out].C;
        }
    nfilters_ = off;
    for (auto& op : ops_)
        if (op.kind == OP_CONV) cast_plan_.add(op.w_off, op.KH * op.KW, tensors_[op.in].C, tensors_[op.out].C);
    for (auto& op : ops_)
        if (op.kind == OP_CONV) {
            op.b_off = off;
            off += tensors_[op.out].C;
        }
    scale_off_ = off;
    off += 512;
    nparams_ = off;

    // ---- variables under the reference's names ------------------------------------------
    auto add_var = [&](const std::string& n, int nd, int s0, int s1, int s2, int s3, size_t o, size_t rows, size_t width,
                       size_t pitch) {
        Variable v;
        v.name = n; v.ndim = nd; v.shape[0] = s0; v.shape[1] = s1; v.shape[2] = s2; v.shape[3] = s3;
        v.off = o; v.rows = rows; v.width = width; v.pitch = pitch;
        vars_.push_back(v);
    };
    for (auto& op : ops_) {
        if (op.kind != OP_CONV) continue;
        const int ci = tensors_[op.in].C, co = tensors_[op.out].C;
        if (op.head < 0) {
            const size_t n = (size_t)op.KH * op.KW * ci * co;
            // the fc graph's two layers keep their scopes (mod_conv6 / mod_conv7) but take the SavedModel's variables
            // (ssdvgg.py:215-228): fc6/weights, fc6/biases, fc7/weights, fc7/biases
            const bool fcv = fc_ && (op.name == "mod_conv6" || op.name == "mod_conv7");
            const std::string vn = fcv ? (op.name == "mod_conv6" ? "fc6" : "fc7") : op.name;
            add_var(vn + (fcv ? "/weights" : "/filter"), 4, op.KH, op.KW, ci, co, op.w_off, 1, n, n);
            add_var(vn + "/biases", 1, co, 0, 0, 0, op.b_off, 1, co, co);
        } else {
            for (int j = 0; j < p.ntypes[op.head]; ++j) {
                const std::string base = "classifiers/classifier" + std::to_string(op.head) + "_" + std::to_string(j);
                add_var(base + "/filter", 4, 3, 3, ci, nv, op.w_off + (size_t)j * nv, (size_t)9 * ci, nv, co);
                add_var(base + "/biases", 1, nv, 0, 0, 0, op.b_off + (size_t)j * nv, 1, nv, nv);
            }
        }
    }
    add_var("l2_norm_conv4_3/scale", 1, 512, 0, 0, 0, scale_off_, 1, 512, 512);
}

// Measurement aid (tools/step_time.py), never set in a product run: ssd_debug_set_ablate("<tokens>") drops groups of launches
// from the step so their price INSIDE the overlapped step can be read off (results are wrong by construction; a warning goes
// to stderr whenever the set changes).  Tokens: pool, tail (conv8_2 ... conv11_2 and the small maps' heads), heads01, conv1,
// conv5, l2norm, reduce (conv_igemm.hip).
static std::string g_ablate;
static std::mutex g_ablate_mu;                     // (set from one thread while another runs a step: the string is never read unlocked)
static std::atomic<bool> g_ablate_on{false};       // the fast path of every launch site: one relaxed load
void set_ablate(const char* tokens) {
    std::lock_guard<std::mutex> lock(g_ablate_mu);
    g_ablate = tokens ? tokens : "";
    g_ablate_on.store(!g_ablate.empty(), std::memory_order_release);
    if (!g_ablate.empty())
        fprintf(stderr, "[ssdvgg_hip] WARNING: ablation '%s' is active: the step SKIPS launches, every result is WRONG (timing aid only)\n",
                g_ablate.c_str());
}
bool ablated(const char* token) {
    if (!g_ablate_on.load(std::memory_order_acquire)) return false;
    std::lock_guard<std::mutex> lock(g_ablate_mu);
    return g_ablate.find(token) != std::string::npos;
}
static bool op_ablated(const std::string& name, int kind, int head, int k) {
    if (!g_ablate_on.load(std::memory_order_acquire)) return false;
    if (kind == 1) return k == 2 && ablated("pool");
    if (kind == 2) return ablated("l2norm");
    if (head >= 2) return ablated("tail");
    if (head >= 0) return ablated("heads01");
    if (name.rfind("conv1_", 0) == 0 && name.size() == 7) return ablated("conv1");
    if (name.rfind("conv5_", 0) == 0) return ablated("conv5");
    if (name.rfind("conv8_2", 0) == 0 || name.rfind("conv9_", 0) == 0 || name.rfind("conv10_", 0) == 0 || name.rfind("conv11_", 0) == 0 ||
        name.rfind("conv12_", 0) == 0)
        return ablated("tail");
    return false;
}

static int env_i(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

// Issue orders.  The op list is the reference's graph order (ssdvgg.py:190-372: trunk, extra layers, l2-norm, classifiers); the
// arena layout and the variables follow it.  What is ISSUED when is a separate matter:
//  * Forward: a branch op (the l2-norm, a fused multibox head) is issued right behind the tensor it reads.  In graph order
//    all of them sat behind conv11_2, and because the heads of a lane share one in-order side stream whose first entry
//    (head 0) needs the l2-norm, the six heads ran back to back AFTER the trunk on a nearly empty chip: 340 us of a
//    7.47 ms bf16 step with fewer than 256 workgroups in flight (profiles/r04_a_timeline_bf16.txt; fp32: 0.6 ms).
//  * Backward: reverse graph order, in bf16 with the big heads behind the chain (below).  (Round 4 built and measured another
//    alternative -- head 0 + l2-norm deferred beside mod_conv6 on the side stream: chain 450 -> 264 us, step 7.22 -> 7.37 ms,
//    profiles/r04_g_ab_schedule_bf16.txt; re-measured in round 5: 6.864 -> 6.885 ms.  The bookkeeping (bw_need / bw_sync /
//    BwProgress) serves any valid order.)
void Net::build_orders() {
    const int n = (int)ops_.size();
    fwd_order_.clear();
    std::vector<char> placed(n, 0);
    std::vector<int> stack;
    for (int i0 = 0; i0 < n; ++i0) {
        if (placed[i0]) continue;
        stack.assign(1, i0);
        while (!stack.empty()) {
            const int i = stack.back();
            stack.pop_back();
            if (placed[i]) continue;
            placed[i] = 1;
            fwd_order_.push_back(i);
            for (int j = n - 1; j > i; --j)      // (pushed in reverse: popped in graph order)
                if (!placed[j] && ops_[j].in == ops_[i].out && (ops_[j].kind == OP_L2NORM || ops_[j].head >= 0)) stack.push_back(j);
        }
    }
    bwd_order_.clear();
    for (int i = n - 1; i >= 0; --i) bwd_order_.push_back(i);
    // (Round 5 ran the bf16 step with the two BIG heads and the l2-norm BEHIND the chain conv11_2 ... conv8_2 -- in graph order their data
    // gradients filled every CU while the chain's first small links were due: 6.864 -> 6.810 ms, profiles/r05_r_ab_bw_defer_bf16.txt.  With
    // round 6's one-launch tail there is no chain of small launches left to starve and graph order measures 0.7 - 0.9 % faster in bf16,
    // equal in fp32 (profiles/r06_bd_ab_bw_order_*.txt, r06_am_ab_bw_defer_sync_bf16.txt): the reordering and its switch are gone.)
    // every op exactly once
    SSD_REQUIRE((int)bwd_order_.size() == n && (int)fwd_order_.size() == n, "issue orders lost an op (%zu forward, %zu backward of %d)",
                fwd_order_.size(), bwd_order_.size(), n);
}

// stream class of an op's data gradient in backward: 0 = main stream, 1 = side stream (see build_orders)
// Round 5: of the small maps' heads only the LAST one's data gradient starts the side chain (conv11_2's needs it); the others'
// (maps 2 .. n-2) run on the MAIN stream in front of the two big heads.  On the one side stream the four of them ran back to back
// -- 200 us at 30-66 us each beside the big heads' kernels -- before conv11_2's data gradient could start, and the main stream then
// waited 316 us for the chain's end (profiles/r05_l_timeline_merged_tail_bf16.txt).  The chain picks their results up through an
// event per feature map (Tensor::gev), not through a join of the streams.
int Net::bw_class(const Op& op, int op_index) const {
    if (!(hstream_ && overlap_)) return 0;
    if (op.kind == OP_CONV && op.head >= 2) return op.head != heads_.nmaps - 1 ? 0 : 1;      // small maps' heads: a few workgroups each
    if (op.kind == OP_CONV && op.head < 0 && op_index > tail_first_) return 1;     // conv11_2 ... conv8_2 behind them
    return 0;
}

void Net::bw_sync(int x, int y) {
    hipEvent_t ev = y == 1 ? ev_h_ : ev_m2s_;
    HIP_OK(hipEventRecord(ev, y == 1 ? hstream_ : stream_));
    HIP_OK(hipStreamWaitEvent(x == 1 ? hstream_ : stream_, ev, 0));
    bwd_.seen[x][y] = bwd_.issued[y];
}

void Net::bw_need(int x, int ti) {
    const BwdPass::Grad& g = bwd_.t[ti];
    if (g.gstream == x || g.gseq <= bwd_.seen[x][g.gstream]) return;
    if (g.gev_set) HIP_OK(hipStreamWaitEvent(x == 1 ? hstream_ : stream_, tensors_[ti].gev, 0));      // exactly the kernel that wrote it
    else bw_sync(x, g.gstream);
}

void Net::bw_wrote(int x, int ti, bool carried) {
    BwdPass::Grad& g = bwd_.t[ti];
    g.gstream = x;
    g.gseq = ++bwd_.issued[x];
    if (hipEvent_t gev = tensors_[ti].gev) {
        if (!carried) HIP_OK(hipEventRecord(gev, x == 1 ? hstream_ : stream_));      // (carried: the kernel's own stop event, common.h)
        g.gev_set = true;
    }
}

// A fresh record: every field at its default, so a field added to BwdPass is reset without a line here.  The two vectors keep their
// storage (assign into a vector of that size already: no allocation from the second pass on).
void Net::BwdPass::begin(const Net* n, int batch) {
    BwdPass fresh;
    fresh.b = batch;
    fresh.progress.done = std::move(progress.done);
    fresh.progress.begin(n);
    fresh.t = std::move(t);
    fresh.t.assign(n->tensors_.size(), Grad{});
    *this = std::move(fresh);
}

void Net::BwProgress::begin(const Net* n) {
    net = n;
    done.assign(n->ops_.size(), 0);
    chain_done = false;
    pos = 0;
    hi = lo = n->nfilters_;
}

// (min_floats = 0 counts as 1: a stage that asked for nothing would run no op, and a caller that loops until the order is exhausted --
// backward_ranges, every staged backward -- would never return)
int Net::BwProgress::next(size_t min_floats) {
    return !finished() && hi - lo < std::max<size_t>(min_floats, 1) ? net->bwd_order_[pos++] : -1;
}

bool Net::BwProgress::finished() const { return pos >= (int)net->bwd_order_.size(); }

size_t Net::BwProgress::final_lo() const {
    size_t f = net->nfilters_;
    for (int i = (int)net->ops_.size() - 1; i >= 0; --i) {
        if (net->ops_[i].kind != OP_CONV) continue;
        if (!done[i]) break;
        f = net->ops_[i].w_off;      // conv ops own descending, adjacent filter ranges
    }
    return f;
}

// The chain rule (plan_tail_chain): the chain's weight gradients are one grouped launch, issued when backward meets the chain's first
// member in its order -- all of them but chain_first_'s, which keeps its own launch and retires when its turn comes.
void Net::BwProgress::retire_chain() {
    for (size_t j = 0; j < net->ops_.size(); ++j)
        if (net->in_chain_[j] && (int)j != net->chain_first_) done[j] = 1;
    chain_done = true;
    lo = final_lo();
}

size_t Net::BwProgress::retire(int op_index) {
    const Op& op = net->ops_[op_index];
    if (op.kind != OP_CONV) return lo;
    if (net->chain_bwd_ && net->in_chain_[op_index] && !op_ablated(op.name, op.kind, op.head, op.k)) {
        if (!chain_done) retire_chain();
        if (op_index != net->chain_first_) return lo;
    }
    done[op_index] = 1;
    return lo = final_lo();
}

std::pair<size_t, size_t> Net::BwProgress::end_stage() {
    const std::pair<size_t, size_t> r(lo, hi - lo);
    hi = lo;
    return r;
}

// Pool fusion (round 5).  A 2x2 stride-2 pool whose input has no other consumer (pool1-3: conv4_3 also feeds the l2-norm) is
// pure HBM traffic between two convolutions: forward reads the producer's output once more to write a quarter of it, backward
// reads the consumer's data gradient once more to write four times as much.  Where the kernels support it
//  * the PRODUCER's forward epilogue takes the maxima and writes the pooled tensor and the pool's record; its own output is
//    then never written -- nothing reads it in backward either (the record carries the argmax and the relu sign);
//  * the CONSUMER's data gradient scatters through the record straight into the producer's output gradient.
// SSD_POOL_FUSE: bit 0 forward, bit 1 backward, bit 2 (bf16) conv1_1's weight gradient inside conv1_2's data gradient
// (dgrad_first_wgrad); default 7; 0 = the separate kernels, for the A/B and the identity checks.
void Net::plan_pool_fusion() {
    const int mode = env_i("SSD_POOL_FUSE", 7);      // (read per handle: the tests build a fused and an unfused handle in one process)
    fuse_first_wgrad_ = (mode & 4) != 0 && bf16_ && training_;
    first_conv_ = -1;      // the layer whose weight gradient that is: the convolution that reads the image (dgrad_first_wgrad)
    for (int i = 0; i < (int)ops_.size(); ++i)
        if (ops_[i].kind == OP_CONV && ops_[i].in == input_t_) first_conv_ = i;
    for (int i = 0; i < (int)ops_.size(); ++i) {
        Op& pl = ops_[i];
        if (pl.kind != OP_POOL) continue;
        const Tensor& in = tensors_[pl.in];
        const Tensor& out = tensors_[pl.out];
        PoolDesc pd{Bmax_, in.H, in.W, in.C, out.H, out.W, pl.k, pl.stride, pl.pad_h, pl.pad_w};
        if (!maxpool_rec_applicable(pd) || in.consumers != 1 || out.consumers != 1) continue;
        int prod = -1, cons = -1;
        for (int j = 0; j < (int)ops_.size(); ++j) {
            if (ops_[j].out == pl.in) prod = j;
            if (ops_[j].in == pl.out) cons = j;
        }
        if (prod < 0 || cons < 0 || ops_[prod].kind != OP_CONV || ops_[cons].kind != OP_CONV) continue;
        if (!ops_[prod].relu || ops_[prod].head >= 0) continue;
        if (pl.fp8 || ops_[prod].fp8) continue;      // (fp8 handle: a pool on e4m3 bytes / behind an fp8 layer is a launch of its own)
        const ConvDesc dp = conv_desc(ops_[prod], Bmax_), dc = conv_desc(ops_[cons], Bmax_);
        const bool in_bf16 = bf16_ && !tensors_[ops_[prod].in].data_f32;
        if ((mode & 1) && (bf16_ ? (in_bf16 && conv_fwd_pool_bf16_supported(dp)) : conv_fwd_pool_supported(dp))) {
            ops_[prod].pool_after = i;
            pl.fused_fwd = true;
        }
        if ((mode & 2) && training_ && pl.pool_rec && (bf16_ ? conv_dgrad_unpool_bf16_supported(dc) : conv_dgrad_unpool_supported(dc))) {
            ops_[cons].unpool = i;
            pl.fused_bwd = true;
        }
    }
}

// Round 6, the tail as one launch per direction (bf16; conv.h TailStage, tail_bf16.hip).  The chain starts at the first 1x1
// "convN_1" layer behind conv8_2 whose input map is at most 10 x 10 -- below that a layer is a tile or two per image and nothing
// couples two images -- and holds every extra layer from there on plus the multibox heads that read their outputs:
//   forward   conv9_1, conv9_2, head3, conv10_1, conv10_2, head4, conv11_1, conv11_2, head5                    (vgg300)
//   backward  data gradients of head5, head4, head3, conv11_2, conv11_1, conv10_2, conv10_1, conv9_2 in ONE launch (the first
//             layer's own data gradient accumulates into a tensor the 10x10 head also writes: it stays a launch), then the
//             weight gradients of the other eight layers in ONE grouped launch with a direct epilogue (no slabs, no reduces);
//             the first layer keeps its own weight-gradient launch and slab reduce.
// 27 launches of round 5 (9 forward, 8 + 10 backward, not counting 9 reduces) become 3 (+ one that packs the filters).
// SSD_TAIL_FUSE: bit 0 forward, bit 1 backward; default 3; 0 = the per-layer launches.
void Net::plan_tail_chain() {
    chain_first_ = -1;
    in_chain_.assign(ops_.size(), 0);
    const int mode = env_i("SSD_TAIL_FUSE", 3);      // (read per handle) bit 0: forward, bit 1: backward
    chain_fwd_ = chain_bwd_ = false;
    if (!bf16_ || (mode & 3) == 0) return;
    const int n = (int)ops_.size();
    for (int i = tail_first_ + 1; i < n; ++i) {
        const Op& op = ops_[i];
        if (op.kind != OP_CONV || op.head >= 0) continue;
        const Tensor& in = tensors_[op.in];
        if (op.KH == 1 && op.KW == 1 && in.H * in.W <= 100) { chain_first_ = i; break; }
    }
    if (chain_first_ < 0) return;
    std::vector<char> produced(tensors_.size(), 0);
    int count = 0;
    for (int i = chain_first_; i < n; ++i) {
        const Op& op = ops_[i];
        if (op.kind != OP_CONV) continue;
        const bool member = op.head < 0 ? true : produced[op.in] != 0;      // the extra layers; the heads that read one of them
        if (!member) continue;
        if (!tail_chain_stage_supported(conv_desc(op, 1)) || tensors_[op.in].data_f32) { count = -1; break; }
        in_chain_[i] = 1;
        if (op.head < 0) produced[op.out] = 1;
        ++count;
    }
    if (count < 2 || count > tail_chain_max_stages() || count > conv_wgrad_group_bf16_max()) {
        chain_first_ = -1;
        in_chain_.assign(ops_.size(), 0);
        return;
    }
    // the chain kernel reads its filters in fragment order (one contiguous KB per wave and k step): a third image of these few
    // layers' filters, refreshed with the bf16 mirrors every forward pass
    tail_fwd_off_.assign(ops_.size(), -1);
    tail_bwd_off_.assign(ops_.size(), -1);
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (!in_chain_[i]) continue;
        const ConvDesc d = conv_desc(ops_[i], 1);
        tail_fwd_off_[i] = (long long)total;
        total += tail_chain_packed_elems(d, false);
        if (training_ && i != chain_first_) {
            tail_bwd_off_[i] = (long long)total;
            total += tail_chain_packed_elems(d, true);
        }
    }
    wq_tail_ = (bf16_t*)hip_.mem(total * 2);
    chain_fwd_ = (mode & 1) != 0;
    chain_bwd_ = (mode & 2) != 0 && training_;
}

void Net::pack_tail_filters(hipStream_t s) {
    std::vector<TailPackItem> items;
    for (int i = 0; i < (int)ops_.size(); ++i) {
        if (!in_chain_[i]) continue;
        const ConvDesc d = conv_desc(ops_[i], 1);
        items.push_back(TailPackItem{d, false, wq_oi_ + ops_[i].w_off, wq_tail_ + tail_fwd_off_[i]});
        if (tail_bwd_off_[i] >= 0) items.push_back(TailPackItem{d, true, wq_io_ + ops_[i].w_off, wq_tail_ + tail_bwd_off_[i]});
    }
    tail_chain_pack_filters(items.data(), (int)items.size(), s);
}

void Net::launch_tail_forward(int b0, int nb, hipStream_t s) {
    std::vector<TailStage> st;
    for (const int oi : fwd_order_) {
        if (!in_chain_[oi]) continue;
        const Op& op = ops_[oi];
        const Tensor& in = tensors_[op.in];
        const Tensor& out = tensors_[op.out];
        TailStage t{};
        t.d = conv_desc(op, 1);
        t.dgrad = false;
        t.src = static_cast<const char*>(in.data) + (size_t)b0 * in.per_image() * 2;
        t.wgt_packed = wq_tail_ + tail_fwd_off_[oi];
        t.bias = params_ + op.b_off;
        t.dst = static_cast<char*>(out.data) + (size_t)b0 * out.per_image() * (out.data_f32 ? 4 : 2);
        t.relu = op.relu; t.accum = false; t.out_f32 = out.data_f32;
        st.push_back(t);
    }
    prof_.layer = "tail";
    tail_chain_bf16(st.data(), (int)st.size(), nb, "tail_fwd_bf16", s, tail_tables_);
}

// The chain's part of backward (see plan_tail_chain): called when backward_step meets the chain's first op in its order.
void Net::launch_tail_backward() {
    const int b = bwd_.b;
    const bool side = hstream_ && overlap_;
    const int cls = side ? 1 : 0;
    hipStream_t ds = cls == 1 ? hstream_ : stream_;
    std::vector<TailStage> st;
    std::vector<int> written;
    const int first_out = ops_[chain_first_].out;      // the gradient the first layer's own data gradient (a launch) reads
    for (const int oi : bwd_order_) {
        if (!in_chain_[oi] || oi == chain_first_) continue;
        const Op& op = ops_[oi];
        const Tensor& in = tensors_[op.in];
        const Tensor& out = tensors_[op.out];
        int& done = bwd_.t[op.in].done;
        bw_need(cls, op.out);                                   // (the loss gradient of the heads: main stream)
        const bool last = done + 1 == in.consumers;
        TailStage t{};
        t.d = conv_desc(op, 1);
        t.dgrad = true;
        t.src = out.grad;
        t.wgt_packed = wq_tail_ + tail_bwd_off_[oi];
        t.mask = (last && in.relu_out) ? in.data : nullptr;
        t.dst = in.grad;
        t.accum = done > 0;
        st.push_back(t);
        done++;
        if (std::find(written.begin(), written.end(), op.in) == written.end()) written.push_back(op.in);
    }
    prof_.layer = "tail";
    const hipEvent_t carry = tensors_[first_out].gev;
    g_stop_event = carry;
    {
        struct Disarm { ~Disarm() { g_stop_event = nullptr; } } disarm;
        tail_chain_bf16(st.data(), (int)st.size(), b, "tail_dgrad_bf16", ds, tail_tables_);
    }
    for (const int ti : written) {      // one kernel wrote them all: the carried event (if any) stands for every one of them
        BwdPass::Grad& g = bwd_.t[ti];
        g.gstream = cls;
        g.gseq = ++bwd_.issued[cls];
        g.gev_set = false;
    }
    if (carry) bwd_.t[first_out].gev_set = true;
    // ---- the weight gradients of every layer of the chain, one launch behind the data gradients
    const bool wside = wstream_ && overlap_;
    hipStream_t ws = wside ? wstream_ : stream_;
    if (wside || cls == 1) {
        wgrad_wait(ws, carry, ds);
        if (!wside) bwd_.seen[0][1] = bwd_.issued[1];      // (the main stream has now waited for the side stream's chain)
    }
    // (the chain's first layer, on the 10x10 map -- 3200 pixels at batch 32 -- would be the group's straggler with its single pixel
    // split: 50 iterations on 8 workgroups; it keeps its own launch and slab reduce, issued when its turn comes)
    std::vector<WgradGroupItem> items;
    for (int oi = 0; oi < (int)ops_.size(); ++oi) {
        if (!in_chain_[oi]) continue;
        const Op& op = ops_[oi];
        const Tensor& in = tensors_[op.in];
        const Tensor& out = tensors_[op.out];
        WgradGroupItem it{};
        it.d = conv_desc(op, b);
        if (oi == chain_first_) continue;      // (whatever the batch: BwProgress::retire_chain, which knows no batch, leaves it out too)
        it.x = in.h(); it.dy = out.gh();
        it.dw = grads_ + op.w_off; it.dbias = grads_ + op.b_off; it.w = params_ + op.w_off;
        items.push_back(it);
    }
    conv_wgrad_group_bf16(items.data(), (int)items.size(), wd_, ws);
    bwd_.progress.retire_chain();
    if (wside) bwd_.side_used = true;
}

// Round 6 (fp32): which layers take the Winograd form (conv.h wino_*).  SSD_WINOGRAD = bits 0 forward / 1 data gradient / 2 weight
// gradient / 3 the big maps' multibox heads too (default 15; the weight gradient reads the forward's transform of the layer's input, so bit 2 needs bit 0);
// SSD_WINO_MIN_CC = the smallest Ci * Co that takes it (default 4096: conv1_2 and up).  The transforms move 2.25x the activations per
// pass and the 36 GEMMs have k = the channel count: at 64 -> 64 channels they are HBM-bound (16 FLOP per byte), and only with 64-wide
// tiles does conv1_2 beat its direct kernels -- 1.55 / 1.65 / 1.14 ms forward / data / weight gradient against 1.95 / 1.91 / 2.04
// (profiles/r06_aw_bench_conv_narrow_tiles.txt; with 128-wide tiles, half of them zeros: 1.90 / 2.18 / 2.2,
// profiles/r06_ao_per_layer_f32_wino_all.txt).  The trunk's 3x3 / stride 1 / SAME layers with Ci in multiples of 32.
void Net::plan_winograd() {
    if (bf16_) return;
    const int mode = env_i("SSD_WINOGRAD", 15), min_cc = env_i("SSD_WINO_MIN_CC", 4096), head_min_hw = env_i("SSD_WINO_HEAD_MIN_HW", 16);
    if (!(mode & 7)) return;
    size_t m_max = 0, v_max = 0, yt_max = 0, xw_max = 0, slab_max = 0;
    bool dual_any = false;
    for (Op& op : ops_) {
        if (op.kind != OP_CONV) continue;
        const ConvDesc d = conv_desc(op, Bmax_);
        if (!wino_applicable(d) || d.Ci * d.Co < min_cc) continue;
        // the fc graph's map-1 head reads 4096 channels: its input transform would be 2.25 x that 19x19 tensor (472 MB at vgg300
        // b32) per training handle -- it keeps the direct kernels
        if (d.Ci > 1024) continue;
        // the multibox heads of the big maps (38x38 / 19x19; vgg512: 64x64 ... 16x16): below that a layer is a handful of tiles
        // whose three launches cost more than the one they replace
        if (op.head >= 0 && (d.Ho < head_min_hw || !(mode & 8))) continue;
        op.wino_f = (mode & 1) != 0;
        op.wino_d = (mode & 2) != 0 && training_ && op.in != input_t_;
        op.wino_w = (mode & 4) != 0 && training_ && op.wino_f;
        if (!(op.wino_f || op.wino_d)) continue;
        const size_t u = (size_t)36 * d.Ci * d.Co, uf = (size_t)36 * d.Ci * wino_kpad(d.Co), t = (size_t)36 * wino_tiles(d);
        if (op.wino_f) {
            op.wino_U = (float*)hip_.mem(u * sizeof(float));
            // the input's transform: kept per layer by a training handle (the weight gradient reads it), per-stream scratch otherwise
            if (training_) op.wino_V = (float*)hip_.mem(t * d.Ci * sizeof(float));
            else v_max = std::max(v_max, t * d.Ci);
            m_max = std::max(m_max, t * d.Co);
        }
        if (op.wino_f && op.wino_d) op.wino_bits = hip_.mem((size_t)wino_tiles(d) * (d.Ci / 4) * 8);      // (against the fp32 mask: 23.47 -> 23.02 ms, profiles/r06_be_*)
        if (op.wino_d) {
            op.wino_Uf = (float*)hip_.mem(uf * sizeof(float));
            HIP_OK(hipMemset(op.wino_Uf, 0, uf * sizeof(float)));      // (rows Co ... kpad(Co) - 1 of every position stay zero)
            yt_max = std::max(yt_max, t * wino_kpad(d.Co));
            xw_max = std::max(xw_max, t * d.Ci);
        }
        if (op.wino_w) {
            yt_max = std::max(yt_max, t * wino_kpad(d.Co));
            for (int b = 1; b <= Bmax_; ++b) slab_max = std::max(slab_max, wino_wgrad_ws_floats(conv_desc(op, b)));
        }
        // (the first Winograd layer's forward transform is a launch of its own: the lanes wait for a 16 KB filter, not for all of them)
        (wino_plan_first_.n == 0 && op.wino_f ? wino_plan_first_ : wino_plan_).add(params_ + op.w_off, op.wino_U, nullptr, d.Ci, d.Co);
        if (op.wino_Uf) wino_plan_flip_.add(params_ + op.w_off, nullptr, op.wino_Uf, d.Ci, d.Co);
        wino_any_f_ |= op.wino_f;
        wino_any_d_ |= op.wino_d;
        dual_any |= op.wino_d && op.wino_w;
    }
    if (wino_plan_.n + wino_plan_first_.n + wino_plan_flip_.n == 0) return;
    ev_wino_ = hip_.event();
    ev_wino_first_ = hip_.event();
    ev_wino_flip_ = hip_.event();
    if (m_max) for (int l = 0; l < 3; ++l) wino_m_[l] = (float*)hip_.mem(m_max * sizeof(float));
    if (v_max) for (int l = 0; l < 3; ++l) wino_vs_[l] = (float*)hip_.mem(v_max * sizeof(float));
    if (training_) {
        wino_yt_ = (float*)hip_.mem(yt_max * sizeof(float));
        wino_xw_ = (float*)hip_.mem(xw_max * sizeof(float));
        wino_ya_ = (float*)hip_.mem(yt_max * sizeof(float));
        wino_slab_ = (float*)hip_.mem(slab_max * sizeof(float));
        // a layer with both gradients in this form: its dy is transformed once, on the main stream, into wino_ya_ / wino_ya2_ in turn
        // (wgrad_handoff) -- the second buffer is yt_max floats more (1.66 GB at vgg300 batch 32)
        if (dual_any) {
            wino_ya2_ = (float*)hip_.mem(yt_max * sizeof(float));
            for (hipEvent_t& e : ev_ya_free_) e = hip_.event();
        }
    }
}

// fp8 handle.  Eligible: a trunk convolution in front of conv8_1 (no multibox head, not in the tail chain) that
// reads an activation (not the image), has Ci % 64 == 0 and is of a shape on which the fp8 kernel measured faster than the bf16 one
// (conv_fwd_fp8_worthwhile) -- a-trous graph: conv3_2 ... conv5_3, mod_conv6, mod_conv7.  A layer with more than 9 taps (the fc
// graph's 7x7 mod_conv6) runs on conv_bigk_fwd_fp8 where conv_bigk_fwd_fp8_worthwhile says so (SSD_FP8_BIGK; an mxfp8 handle: on conv_bigk_fwd_mxfp8 where
// conv_bigk_fwd_mxfp8_worthwhile says so, SSD_MXFP8_BIGK); otherwise it stays on
// conv_bigk_fwd_bf16 with a quantise pass behind it.  A tensor read by such a layer is kept as
// e4m3 (data8).  A pool between two fp8 layers runs on the bytes and its output shares its input's scale.  Where the e4m3 form is
// needed behind a bf16 producer (conv3_1's output in the a-trous graph) a quantise pass of its own makes it.  A tensor with any non-fp8 reader (conv4_3: the l2 norm; mod_conv7's output: its head and conv8_1) keeps its
// bf16 form as well (wants16).  Runs before plan_pool_fusion, which leaves the fp8 layers' pools alone.
// An mxfp6 handle (Quant::mxfp6) takes the mxfp8 plan for up to 9 taps -- the same eligibility, on conv_fwd_mxfp6 -- and leaves a layer
// with more on conv_bigk_fwd_bf16; its filter images and their block scales get arenas of their own (Op::w8_off, Op::sw_off in bytes).
void Net::plan_fp8() {
    size_t nsw = 0;
    for (Tensor& t : tensors_) t.wants16 = false;
    std::vector<int> producer(tensors_.size(), -1);
    for (int i = 0; i < (int)ops_.size(); ++i) {
        Op& op = ops_[i];
        producer[op.out] = i;
        if (op.kind != OP_CONV) continue;
        const ConvDesc d = conv_desc(op, Bmax_);
        // (mxfp8: the fc graph's fc6 stays on bf16 with a quantise pass behind it unless SSD_MXFP8_BIGK=1 -- conv_bigk_fwd_mxfp8_worthwhile;
        // asked with the most demanding output mode, so that whichever form the readers below take can be launched)
        // (mxfp6: the mxfp8 handle's layers up to 9 taps -- the same Ci % 64, Co % 8 contract -- and nothing above: no mxfp6 kernel for more)
        const bool kernel8 = !conv_bigk(d) ? conv_fwd_fp8_supported(d, nullptr) && conv_fwd_fp8_worthwhile(d) && (quant_ != Quant::mxfp6 || conv_fwd_mxfp6_supported(d, nullptr))
                             : quant_ == Quant::mxfp6 ? false
                             : quant_ == Quant::mxfp8 ? conv_bigk_fwd_mxfp8_supported(d, FP8_OUT_BF16_MX, nullptr) && conv_bigk_fwd_mxfp8_worthwhile(d)
                                                      : conv_bigk_fwd_fp8_supported(d, nullptr) && conv_bigk_fwd_fp8_worthwhile(d);
        op.fp8 = op.head < 0 && i < tail_first_ && !tensors_[op.in].data_f32 && kernel8;
    }
    auto need8 = [&](Tensor& t) {
        // One byte per element, whatever the kind: an mxfp6 tensor takes quant_code_bytes() of it, three quarters.  The size is kept:
        // which bytes past a format's nominal end its kernels touch has not been checked on a GPU.
        if (!t.data8) t.data8 = static_cast<unsigned char*>(hip_.mem(t.per_image() * Bmax_));
        // (+ 8: conv_fwd_mxfp8 and conv_fwd_mxfp6 read the scales in whole dwords)
        if (quant_block_scales(quant_) && !t.scale8)
            t.scale8 = static_cast<unsigned char*>(hip_.mem(quant_scale_bytes(quant_, t.per_image()) * Bmax_ + 8));
    };
    for (int i = (int)ops_.size() - 1; i >= 0; --i) {      // readers before their producers: a pool learns from its consumer
        Op& op = ops_[i];
        Tensor& in = tensors_[op.in];
        Tensor& out = tensors_[op.out];
        if (op.kind == OP_POOL) {
            const int prod = producer[op.in];
            op.fp8 = out.data8 != nullptr && prod >= 0 && ops_[prod].kind == OP_CONV && ops_[prod].fp8;
            if (op.fp8) {
                need8(in);
                if (out.wants16) in.wants16 = true;      // the bf16 pool beside it needs its bf16 input
            } else {
                in.wants16 = true;
            }
        } else if (op.kind == OP_CONV && op.fp8) {
            need8(in);
        } else {
            in.wants16 = true;
        }
    }
    for (int t : head_t_) tensors_[t].wants16 = true;      // (fp32, read by the loss / result pass)
    size_t nw6 = 0;      // mxfp6: bytes of code images so far; every image and scale table starts at a multiple of 16 bytes
    for (Op& op : ops_) {
        if (op.kind == OP_CONV && op.fp8 && quant_ == Quant::mxfp6) {
            const Tensor& in = tensors_[op.in];
            const Tensor& out = tensors_[op.out];
            const size_t n = (size_t)op.KH * op.KW * out.C * in.C;      // (blocks along Ci, a multiple of 64)
            op.sw_off = nsw;
            op.w8_off = nw6;
            quant_plan_.add(op.w_off, nw6, nsw, op.KH * op.KW, in.C, out.C);
            nw6 += (quant_code_bytes(quant_, n) + 15) / 16 * 16;
            nsw += (quant_scale_bytes(quant_, n) + 15) / 16 * 16;
        } else if (op.kind == OP_CONV && op.fp8) {
            const Tensor& in = tensors_[op.in];
            const Tensor& out = tensors_[op.out];
            op.sw_off = nsw;
            op.w8_off = op.w_off;
            quant_plan_.add(op.w_off, op.w8_off, nsw, op.KH * op.KW, in.C, out.C);
            nsw += out.C;
        }
        Tensor& out = tensors_[op.out];
        if (!out.data8) continue;
        if (!op.fp8) out.wants16 = true;      // a bf16 op writes bf16; the quantise pass behind it makes the e4m3 form
        if (!(op.kind == OP_POOL && op.fp8) && quant_tensor_scale(quant_)) fp8_scaled_.push_back(op.out);      // (MX kinds: no tensor owns a scale)
    }
    SSD_REQUIRE(quant_plan_.n > 0, "no layer of this graph is eligible for fp8");
    if (quant_ == Quant::mxfp6) {      // (+ 8: conv_fwd_mxfp6 reads the scales in whole dwords)
        w8_ = static_cast<unsigned char*>(hip_.mem(nw6));
        wsc6_ = static_cast<unsigned char*>(hip_.mem(nsw + 8));
        return;
    }
    w8_ = static_cast<unsigned char*>(hip_.mem(nfilters_));
    sw8_ = static_cast<float*>(hip_.mem(nsw * sizeof(float)));
    if (quant_tensor_scale(quant_)) absmax8_ = static_cast<float*>(hip_.mem(fp8_scaled_.size() * sizeof(float)));
}

QView Net::q_at(const Tensor& t, int b0) const {
    return QView{t.data8 ? t.data8 + (size_t)b0 * quant_code_bytes(quant_, t.per_image()) : nullptr,
                 t.scale8 ? t.scale8 + (size_t)b0 * quant_scale_bytes(quant_, t.per_image()) : nullptr, t.scale};
}

void Net::require_fp8() const {
    SSD_REQUIRE(quant_ != Quant::mxfp6, "an mxfp6 handle has no calibration scales (SSD_DTYPE_MXFP6): every producer chooses its block scales itself");
    SSD_REQUIRE(quant_ != Quant::mxfp8, "an mxfp8 handle has no calibration scales (SSD_DTYPE_MXFP8): every producer chooses its block scales itself");
    SSD_REQUIRE(quant_ == Quant::fp8, "not an fp8 handle (SSD_DTYPE_FP8)");
}

void Net::fp8_share_pool_scales() {
    for (const Op& op : ops_)      // graph order: a pool comes behind its input's producer
        if (op.kind == OP_POOL && op.fp8) tensors_[op.out].scale = tensors_[op.in].scale;
}

int Net::fp8_num_scales() const {
    require_fp8();
    return (int)fp8_scaled_.size();
}

const char* Net::fp8_scale_name(int i) const {
    require_fp8();
    SSD_REQUIRE(i >= 0 && i < (int)fp8_scaled_.size(), "fp8 scale index %d outside 0..%zu", i, fp8_scaled_.size() - 1);
    return tensors_[fp8_scaled_[i]].name.c_str();
}

void Net::fp8_get_scales(float* out, int n) const {
    require_fp8();
    SSD_REQUIRE(out && n == (int)fp8_scaled_.size(), "the handle has %zu fp8 scales, got room for %d", fp8_scaled_.size(), n);
    for (int i = 0; i < n; ++i) out[i] = tensors_[fp8_scaled_[i]].scale;
}

void Net::fp8_set_scales(const float* v, int n) {
    require_fp8();
    if (!v || n != (int)fp8_scaled_.size()) {      // (e.g. scales saved from another plan: SSD_FP8_BIGK moves the fc graph's)
        std::string names;
        for (int t : fp8_scaled_) names += (names.empty() ? "" : ", ") + tensors_[t].name;
        SSD_REQUIRE(false, "the handle has %zu fp8 scales (%s), got %d", fp8_scaled_.size(), names.c_str(), n);
    }
    for (int i = 0; i < n; ++i)
        SSD_REQUIRE(v[i] > 0.f && v[i] < INFINITY, "fp8 scale %d (%s) must be positive and finite, got %g", i, fp8_scale_name(i), (double)v[i]);
    HIP_OK(hipStreamSynchronize(stream_));      // (no pass in flight reads a scale: they travel as kernel arguments; this orders the caller's view)
    for (int i = 0; i < n; ++i) tensors_[fp8_scaled_[i]].scale = v[i];
    fp8_share_pool_scales();
    fp8_calibrated_ = true;
}

// The handle's graph on the bf16 kernels, then the absmax of every scaled tensor's bf16 form: scale = max(absmax, tiny) / 448,
// with `accumulate` the larger of that and the scale already there.
void Net::fp8_calibrate(const float* x_dev, int b, bool accumulate) {
    require_fp8();
    struct Scope {
        bool& f;
        Scope(bool& f_) : f(f_) { f = true; }
        ~Scope() { f = false; }
    } scope(fp8_as_bf16_);
    forward(x_dev, b, false, nullptr);
    const int n = (int)fp8_scaled_.size();
    for (int i = 0; i < n; ++i) {
        const Tensor& t = tensors_[fp8_scaled_[i]];
        absmax_bf16(t.h(), (size_t)b * t.per_image(), absmax8_ + i, false, stream_);
    }
    std::vector<float> am(n);
    HIP_OK(hipMemcpyAsync(am.data(), absmax8_, n * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_OK(hipStreamSynchronize(stream_));
    constexpr float tiny = 1e-20f;
    for (int i = 0; i < n; ++i) {
        Tensor& t = tensors_[fp8_scaled_[i]];
        const float s = std::max(am[i], tiny) / 448.0f;
        t.scale = (accumulate && fp8_calibrated_) ? std::max(t.scale, s) : s;
    }
    fp8_share_pool_scales();
    fp8_calibrated_ = true;
}

void Net::pool_fusion(int* out, int cap, int* count) const {
    int k = 0;
    for (const Op& op : ops_)
        if (op.kind == OP_POOL && op.k == 2 && op.stride == 2) {
            if (out && k < cap) out[k] = (op.fused_fwd ? 1 : 0) | (op.fused_bwd ? 2 : 0);
            ++k;
        }
    if (count) *count = k;
}

size_t Net::arena_floats(const char* preset, int num_classes, int graph) {
    // cheap: build the graph description only
    const Preset& p = get_preset(preset);
    require_num_classes(num_classes);
    SSD_REQUIRE(graph == 0 || graph == 1, "graph must be 0 (a-trous) or 1 (fc), got %d", graph);
    const int nv = num_classes + 5;
    const int c7 = graph == 1 ? 4096 : 1024;      // mod_conv7's width: the input of conv8_1 and of the map-1 head
    size_t n = 0;
    auto cv = [&](int k, int ci, int co) { n += (size_t)k * k * ci * co + co; };
    cv(3, 3, 64); cv(3, 64, 64); cv(3, 64, 128); cv(3, 128, 128); cv(3, 128, 256); cv(3, 256, 256); cv(3, 256, 256);
    cv(3, 256, 512); cv(3, 512, 512); cv(3, 512, 512); cv(3, 512, 512); cv(3, 512, 512); cv(3, 512, 512);
    if (graph == 1) { cv(7, 512, 4096); cv(1, 4096, 4096); }
    else { cv(3, 512, 1024); cv(1, 1024, 1024); }
    cv(1, c7, 256); cv(3, 256, 512); cv(1, 512, 128); cv(3, 128, 256); cv(1, 256, 128); cv(3, 128, 256);
    cv(1, 256, 128); cv(3, 128, 256);
    if (p.nmaps >= 7) { cv(1, 256, 128); cv(3, 128, 256); }
    const int fch[] = {512, c7, 512, 256, 256, 256, 256};
    for (int i = 0; i < p.nmaps; ++i) cv(3, fch[i], head_ld(p.ntypes[i], nv));
    return n + 512;
}

ConvDesc Net::conv_desc(const Op& op, int b) const {
    const Tensor& in = tensors_[op.in];
    const Tensor& out = tensors_[op.out];
    ConvDesc d;
    d.B = b; d.Hi = in.H; d.Wi = in.W; d.Ci = in.C; d.Ho = out.H; d.Wo = out.W; d.Co = out.C;
    d.KH = op.KH; d.KW = op.KW; d.stride = op.stride; d.dil = op.dil; d.pad_h = op.pad_h; d.pad_w = op.pad_w;
    return d;
}

void Net::alloc() {
    const int B = Bmax_;
    const int nv = C_ + 5;
    const int A = preset_->num_anchors;
    for (size_t i = 0; i < tensors_.size(); ++i) {
        Tensor& t = tensors_[i];
        if ((int)i == input_t_) continue;
        t.data = hip_.mem(t.per_image() * B * (t.data_f32 ? 4 : 2));
        HIP_OK(hipMemset(t.data, 0, t.per_image() * B * (t.data_f32 ? 4 : 2)));
        if (training_) {
            t.grad = hip_.mem(t.per_image() * B * (t.grad_f32 ? 4 : 2));
            HIP_OK(hipMemset(t.grad, 0, t.per_image() * B * (t.grad_f32 ? 4 : 2)));   // head pad columns stay 0 forever
        }
    }
    for (int i = 0; i < heads_.nmaps; ++i) {
        heads_.buf[i] = static_cast<float*>(tensors_[head_t_[i]].data);
        heads_.dbuf[i] = tensors_[head_t_[i]].grad;
    }
    if (bf16_) {
        wq_io_ = (bf16_t*)hip_.mem(nfilters_ * 2);
        wq_oi_ = (bf16_t*)hip_.mem(nfilters_ * 2);
    }
    if (!params_) params_ = (float*)hip_.mem(nparams_ * sizeof(float));
    if (training_) {
        if (!grads_) grads_ = (float*)hip_.mem(nparams_ * sizeof(float));
        if (!mom_) mom_ = (float*)hip_.mem(nparams_ * sizeof(float));
        HIP_OK(hipMemset(grads_, 0, nparams_ * sizeof(float)));
        HIP_OK(hipMemset(mom_, 0, nparams_ * sizeof(float)));
        // split-M slab workspace: one region per layer (the reduces of a backward stage run as one grouped launch at its
        // end, so a layer's slabs must survive the next layer's weight gradient); sized for the worst batch <= B
        size_t ws_total = 0;
        for (auto& op : ops_)
            if (op.kind == OP_CONV) {
                size_t ws = 0;
                for (int b = 1; b <= B; ++b) {
                    const ConvDesc d = conv_desc(op, b);
                    ws = std::max(ws, (bf16_ && d.Ci % 8 == 0) ? conv_wgrad_bf16_ws_floats(d) : conv_wgrad_ws_floats(d));
                    if (bf16_ && first_layer_kernel(d)) ws = std::max(ws, std::max(conv_first_wgrad_bf16_ws_floats(d), conv_dgrad_first_wgrad_bf16_ws_floats(d)));
                }
                op.ws_off = ws_total;
                ws_total += (ws + 63) / 64 * 64;
            }
        wgrad_ws_ = (float*)hip_.mem(ws_total * sizeof(float));
        l2_ws_ = (float*)hip_.mem(l2norm_bwd_ws_floats(B * 64 * 64, 512) * sizeof(float));
        size_t pws = 0;
        for (auto& op : ops_)
            if (op.kind == OP_POOL) {
                const Tensor& in = tensors_[op.in];
                const Tensor& out = tensors_[op.out];
                PoolDesc d{B, in.H, in.W, in.C, out.H, out.W, op.k, op.stride, op.pad_h, op.pad_w};
                pws = std::max(pws, maxpool_bwd_ws_bytes(d));
            }
        pool_ws_ = hip_.mem(pws);
        // 2x2 pools whose input has no other consumer keep a forward record for their backward (ops.h)
        for (auto& op : ops_)
            if (op.kind == OP_POOL) {
                const Tensor& in = tensors_[op.in];
                const Tensor& out = tensors_[op.out];
                PoolDesc d{B, in.H, in.W, in.C, out.H, out.W, op.k, op.stride, op.pad_h, op.pad_w};
                if (maxpool_rec_applicable(d) && in.consumers == 1) op.pool_rec = hip_.mem(maxpool_rec_bytes(d));
            }
    }
    result_ = (float*)hip_.mem((size_t)B * A * nv * sizeof(float));
    x_stage_ = (float*)hip_.mem((size_t)B * preset_->image_h * preset_->image_w * 3 * sizeof(float));
    y_stage_ = (float*)hip_.mem((size_t)B * A * nv * sizeof(float));
    loss_ws_ = hip_.mem(loss_work_bytes(B, A));
    loss_work_carve(lw_, loss_ws_, B, A);
    HIP_OK(hipMemset(loss_ws_, 0, loss_work_bytes(B, A)));
    // The four losses are written by the loss kernel's final block straight into pinned, device-mapped host memory: a
    // 16-byte device-to-host copy would be a blit kernel of its own on the critical path between the loss and its
    // gradient (12 us of launch gap + the kernel in the rocprofv3 trace, tools/trace_gaps.py).
    // A ring of LOSS_RING such slots (one per forward pass) lets the host read step k - 1's losses while step k runs.
    void* dp = nullptr;
    losses_host_ = static_cast<float*>(hip_.pinned(LOSS_RING * 4 * sizeof(float), &dp));
    for (int i = 0; i < LOSS_RING * 4; ++i) losses_host_[i] = 0.f;
    losses_dev_ = static_cast<float*>(dp);
    lw_.losses = losses_dev_;
    for (int i = 0; i < LOSS_RING; ++i) ev_loss_[i] = hip_.event();
    anchors_dev_ = (double*)hip_.mem((size_t)A * 4 * sizeof(double));
    anchors_abs_dev_ = (int*)hip_.mem((size_t)A * 4 * sizeof(int));
    anchors_device(*preset_, anchors_dev_, anchors_abs_dev_, nullptr);
    // Gradient clipping (apply_gradients), after everything else so that every other buffer sits where it sat without it: the norm
    // pass's partials with the update's scale, and a ring of {norm, factor} per clipped update that the finish kernel writes
    // straight into mapped host memory, like the losses above.
    if (training_) {
        clip_ws_ = hip_.mem(grad_norm_ws_bytes(nparams_));
        clip_host_ = static_cast<float*>(hip_.pinned(LOSS_RING * 2 * sizeof(float), &dp));
        for (int i = 0; i < LOSS_RING * 2; ++i) clip_host_[i] = 0.f;
        clip_dev_ = static_cast<float*>(dp);
        for (int i = 0; i < LOSS_RING; ++i) ev_clip_[i] = hip_.event();
    }
    HIP_OK(hipDeviceSynchronize());
}

// splitmix64 -> uniform [0,1)
static inline double urand(unsigned long long& s) {
    unsigned long long z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

void Net::init_weights(unsigned long long seed) {
    std::vector<float> h(nparams_, 0.f);
    unsigned long long s = seed * 0x2545F4914F6CDD1Dull + 1;
    for (const Variable& v : vars_) {
        if (v.ndim == 4) {   // xavier_initializer (uniform): limit = sqrt(6 / (fan_in + fan_out)), ssdvgg.py:46
            const double fan_in = (double)v.shape[0] * v.shape[1] * v.shape[2];
            const double fan_out = (double)v.shape[0] * v.shape[1] * v.shape[3];
            const double lim = std::sqrt(6.0 / (fan_in + fan_out));
            for (size_t r = 0; r < v.rows; ++r)
                for (size_t c = 0; c < v.width; ++c) h[v.off + r * v.pitch + c] = (float)((urand(s) * 2.0 - 1.0) * lim);
        } else if (v.name == "l2_norm_conv4_3/scale") {
            for (size_t c = 0; c < v.width; ++c) h[v.off + c] = 20.f;   // ssdvgg.py:336
        }
    }
    HIP_OK(hipMemcpy(params_, h.data(), nparams_ * sizeof(float), hipMemcpyHostToDevice));
}

Net::Net(const char* preset, int num_classes, int max_batch, int device, bool training, unsigned long long seed,
         float* ext_params, float* ext_grads, float* ext_momentum, int dtype, int graph)
    : preset_(&get_preset(preset)), C_(num_classes), Bmax_(max_batch), device_(device), training_(training), bf16_(dtype >= 1 && dtype <= 4),
      fc_(graph == 1), quant_(dtype == 2 ? Quant::fp8 : dtype == 3 ? Quant::mxfp8 : dtype == 4 ? Quant::mxfp6 : Quant::none), hip_(device) {
    SSD_REQUIRE(dtype >= 0 && dtype <= 4, "dtype must be 0 (fp32), 1 (bf16), 2 (fp8), 3 (mxfp8) or 4 (mxfp6), got %d", dtype);
    SSD_REQUIRE(!(quant_ != Quant::none && training), "%s is inference only: create the handle with training = 0",
                quant_ == Quant::mxfp6 ? "SSD_DTYPE_MXFP6" : quant_ == Quant::mxfp8 ? "SSD_DTYPE_MXFP8" : "SSD_DTYPE_FP8");
    SSD_REQUIRE(graph == 0 || graph == 1, "graph must be 0 (a-trous) or 1 (fc), got %d", graph);
    require_num_classes(num_classes);
    SSD_REQUIRE(max_batch >= 1, "max_batch must be >= 1");
    HIP_OK(hipSetDevice(device));
    params_ = ext_params; grads_ = ext_grads; mom_ = ext_momentum;
    build_graph();
    alloc();
    init_weights(seed);
    const char* ov = getenv("SSD_OVERLAP_WGRAD");
    overlap_ = !(ov && ov[0] == '0');
    wino_dual_ = env_i("SSD_WINO_DUAL", 1);
    wino_dual_max_c_ = env_i("SSD_WINO_DUAL_MAX_C", wino_dual_max_c_);
    hstream_ = hip_.stream();      // (a high-priority side stream was measured again in round 5: +-0)
    ev_h_ = hip_.event();
    ev_cast_ = hip_.event();

    ev2_h_ = hip_.event();
    ev_l2_ = hip_.event();
    ev_join_ = hip_.event();
    ev_m2s_ = hip_.event();
    for (int i = 0; i < MAX_MAPS; ++i) ev2_fmap_[i] = hip_.event();
    for (int i = 0; i < MAX_MAPS; ++i) ev_fmap_[i] = hip_.event();
    if (training_) {
        wstream_ = hip_.stream();
        ev_dy_ = hip_.event();
        ev_w_ = hip_.event();
    }
    // FEW streams: the hardware runs four queues side by side (ROCm's default GPU_MAX_HW_QUEUES); a fifth
    // active stream is time-multiplexed onto one of them, and which two streams then share a queue depends on creation
    // order.  Measured (gpurun r02_v / r02_w, bf16 step): every stream on its own queue (8 queues) 3075 images/s, the
    // default four queues 4016 (and 3850 for a net created after others in the same process), four STREAMS 4080-4120
    // whatever the queue count.  The second forward lane and the weight gradients are never busy at the same time
    // (forward / backward), so they are ONE stream, and the second lane runs its heads on its own main stream as well: THREE
    // streams beside the caller's measure the same as four (bf16 4142 vs 4081 images/s, r02_w) and leave the fourth queue to
    // a data-parallel caller's collective stream.
    s2_ = training_ ? wstream_ : hip_.stream();
    if (quant_ != Quant::none) plan_fp8();
    plan_pool_fusion();
    plan_tail_chain();
    plan_winograd();
    // Round 5: an event per gradient tensor (round 4: the small heads' feature maps only).  The data-gradient kernel that writes it
    // CARRIES the event (g_stop_event), and the weight-gradient stream / the other class wait for exactly that kernel: no event
    // packet between two data gradients on the main stream, none inside the side chain.
    if (training_)
        for (const Op& op : ops_)
            if (op.in != input_t_ && !tensors_[op.in].gev)
                tensors_[op.in].gev = hip_.event();
    bwd_.begin(this, 0);      // (the record's vectors get their size here)
}

Net::~Net() {
    if (g_prof == &prof_) g_prof = nullptr;
}

// ---------------------------------------------------------------------------------
// steps
// ---------------------------------------------------------------------------------
static char* at(const Tensor& t, int b0, bool grad = false) {      // first element of sample b0
    return static_cast<char*>(grad ? t.grad : t.data) + (size_t)b0 * t.per_image() * ((grad ? t.grad_f32 : t.data_f32) ? 4 : 2);
}

// ---- The quantised kinds: one dispatcher per operation, each on views of its operands (Net::q_at), each the launcher of the format.
// the stand-alone quantise pass behind a bf16 producer: nb samples of t's bf16 form (src) into its quantised form from dst on
static void quantize_q(Quant q, const Tensor& t, const void* src, int nb, QView dst, hipStream_t s) {
    switch (q) {
    case Quant::mxfp6: quantize_mxfp6(src, false, (size_t)nb * t.H * t.W, t.C, dst.codes, dst.scales, s); break;
    case Quant::mxfp8: quantize_mxfp8(src, false, (size_t)nb * t.H * t.W, t.C, dst.codes, dst.scales, s); break;
    case Quant::fp8: quantize_fp8(src, false, (size_t)nb * t.per_image(), dst.scale, dst.codes, s); break;
    case Quant::none: fail("quantize: the handle has no quantised format");
    }
}

// the filter images with their per-channel scales (sw8) or their block scales (wsc6), fresh from the fp32 masters: one launch
static void quantize_filters_q(Quant q, const FilterQuantPlan& plan, const float* w, unsigned char* w8, float* sw8, unsigned char* wsc6, hipStream_t s) {
    if (q == Quant::mxfp6) quantize_filters_mxfp6(plan, w, w8, wsc6, s);
    else quantize_filters_fp8(plan, w, w8, sw8, s);
}

// The convolution on quantised operands; the output in the form(s) its readers take: codes where it has a quantised form (y8), bf16 (y)
// where it has no such form or a reader wants that as well (wants16).  sw / wsc: the layer's per-channel / block filter scales.
static void conv_fwd_q(Quant q, const ConvDesc& d, QView x, const unsigned char* w, const float* sw, const unsigned char* wsc, const float* bias,
                       void* y, QView y8, bool wants16, bool relu, hipStream_t s) {
    const int mx_mode = y8.codes ? (wants16 ? FP8_OUT_BF16_MX : FP8_OUT_MX) : FP8_OUT_BF16;
    switch (q) {
    case Quant::mxfp6:      // e2m3 operands, block scales on both
        conv_fwd_mxfp6(d, x.codes, x.scales, w, wsc, bias, y, y8.codes, y8.scales, mx_mode, relu, s);
        break;
    case Quant::mxfp8:      // e4m3 operands with block scales (more than 9 taps: the fc graph's mod_conv6 under SSD_MXFP8_BIGK=1)
        (conv_bigk(d) ? conv_bigk_fwd_mxfp8 : conv_fwd_mxfp8)(d, x.codes, x.scales, w, sw, bias, y, y8.codes, y8.scales, mx_mode, relu, s);
        break;
    case Quant::fp8:        // e4m3 operands (more than 9 taps: the fc graph's mod_conv6)
        (conv_bigk(d) ? conv_bigk_fwd_fp8 : conv_fwd_fp8)(d, x.codes, w, x.scale, sw, bias, y, y8.codes,
                                                          y8.codes ? (wants16 ? FP8_OUT_BF16_E4M3 : FP8_OUT_E4M3) : FP8_OUT_BF16, y8.scale, relu, s);
        break;
    case Quant::none: fail("convolution: the handle has no quantised format");
    }
}

// max-pooling on the codes: fp8 on the bytes (the output shares the input's scale), the MX kinds on the dequantised cells, with block
// scales of the output's own
static void maxpool_fwd_q(Quant q, const PoolDesc& d, QView x, QView y, hipStream_t s) {
    switch (q) {
    case Quant::mxfp6: maxpool_fwd_mxfp6(d, x.codes, x.scales, y.codes, y.scales, s); break;
    case Quant::mxfp8: maxpool_fwd_mxfp8(d, x.codes, x.scales, y.codes, y.scales, s); break;
    case Quant::fp8: maxpool_fwd_fp8(d, x.codes, y.codes, s); break;
    case Quant::none: fail("max-pool: the handle has no quantised format");
    }
}

// A forward pass that fails after it has taken a slot of the loss ring gives the slot back: its event was never
// recorded, and a reader one step late (get_losses_step) would otherwise be handed a slot of four passes ago.
struct Net::LossSlotGuard {
    long long& seq;
    bool armed = false;
    bool done = false;
    explicit LossSlotGuard(long long& s) : seq(s) {}
    void failed() { if (armed && !done) { --seq; armed = false; } }
    ~LossSlotGuard() { if (armed && !done) --seq; }
};

// where one forward convolution launch runs and on which samples; wino_M set: in the Winograd form, on this scratch
struct Net::ConvRun {
    hipStream_t cs;
    int b0, nb;
    float *wino_M = nullptr, *wino_V = nullptr;
    size_t wino_vps = 0;
    void* wino_bits = nullptr;
};

// Forward runs the op list on up to two LANES: the batch is cut in two halves that walk the network side by side (lane 0
// on the caller's stream + the side stream for its heads, lane 1 with its heads on s2_, which is the
// weight-gradient stream: see the constructor), so that the tail of one half's kernel (its last, partial round of workgroups) is filled by the other half's
// kernel instead of idle CUs.  Measured on one box (SSD_FWD_LANES=1 / 2, gpurun r02): training step +0.5 % fp32 and
// +2.7 % bf16, inference at batch 128 +1.6 %.  Nothing in forward couples the samples except the loss's final
// reduction, which the last per-sample workgroup of either lane performs (ops.hip).
void Net::forward(const float* x, int b, bool train_mode, const float* y) {
    SSD_REQUIRE(b >= 1 && b <= Bmax_, "batch %d outside 1..%d (max_batch)", b, Bmax_);
    SSD_REQUIRE(quant_ != Quant::fp8 || fp8_as_bf16_ || fp8_calibrated_,
                "the fp8 handle has no activation scales yet: call ssd_fp8_calibrate_dev or ssd_fp8_set_scales before inference");
    g_prof = &prof_;
    tensors_[input_t_].data = const_cast<float*>(x);
    pool_arg_op_ = -1;
    ++fwd_serial_;
    fwd_swapped_ = ema_swapped_;
    const bool side = hstream_ && overlap_;
    static const int lanes_env = [] { const char* v = getenv("SSD_FWD_LANES"); return v ? atoi(v) : 0; }();
    const int want_lanes = lanes_env > 0 ? lanes_env : 2;
    const int nl = (want_lanes >= 2 && side && s2_ && b >= 8) ? 2 : 1;
    FwdPass p{{{stream_, hstream_, ev_fmap_, ev_h_, 0, nl == 2 ? (b + 1) / 2 : b, false, false, 0, {}},
               {s2_, s2_, ev2_fmap_, ev2_h_, (b + 1) / 2, b - (b + 1) / 2, false, false, 0, {}}},
              nl, nl, nl == 2, 0, b, train_mode, quant_ != Quant::none && !fp8_as_bf16_, side};
    if (side && (bf16_ || train_mode || nl == 2)) {
        HIP_OK(hipEventRecord(ev_fmap_[MAX_MAPS - 1], stream_));      // everything issued so far (the previous step's update)
        HIP_OK(hipStreamWaitEvent(hstream_, ev_fmap_[MAX_MAPS - 1], 0));
        if (nl == 2) HIP_OK(hipStreamWaitEvent(s2_, ev_fmap_[MAX_MAPS - 1], 0));
        p.lane[0].heads_on_side = true;
    }
    LossSlotGuard fwd_guard(loss_seq_);
    forward_filters(p, fwd_guard);
    // Round 5: the lanes MERGE at conv8_1.  The extra layers behind it are a chain of sixteen dependent launches of a handful of
    // workgroups each (conv8_1 ... conv11_2 on two lanes: 6-37 us per launch, every one of them latency- not work-bound): a
    // timeline of the step (profiles/r05_j_timeline_bf16.txt) shows 285 us between mod_conv7 and the loss with a nearly empty chip.
    // One lane runs the eight layers once, at twice the rows per launch and the same latency; the second lane's stream -- idle
    // from here on -- takes every other small head, which used to queue behind each other on the one side stream.
    // (Round 4 merged at the 19x19 maps, i.e. incl. conv5_x / mod_conv6, where two lanes fill each other's partial rounds: slower.)
    for (const int op_index : fwd_order_) {
        const Op& op = ops_[op_index];
        prof_.layer = op.name.c_str();
        if (op_ablated(op.name, op.kind, op.head, op.k)) continue;
        if (chain_fwd_ && in_chain_[op_index]) {      // Round 6 (plan_tail_chain): the chain's layers and heads run as ONE launch per lane, issued at its first op
            if (op_index == chain_first_)
                for (int li = 0; li < p.nl_cur; ++li) {
                    Lane& ln = p.lane[li];
                    if (ln.cast_pending) {
                        HIP_OK(hipStreamWaitEvent(ln.s, ev_cast_, 0));
                        ln.cast_pending = false;
                    }
                    launch_tail_forward(ln.b0, ln.nb, ln.s);
                }
            continue;
        }
        if (p.nl_cur == 2 && p.heads_full && op_index == tail_first_) {
            HIP_OK(hipEventRecord(ev_join_, s2_));
            HIP_OK(hipStreamWaitEvent(stream_, ev_join_, 0));
            p.lane[0].nb = b;
            p.nl_cur = 1;
        }
        for (int li = 0; li < p.nl_cur; ++li)
            switch (op.kind) {
            case OP_CONV: forward_conv(p, li, op_index); break;
            case OP_POOL: forward_pool(p, li, op_index); break;
            case OP_L2NORM: forward_l2norm(p, li, op_index); break;
            }
    }
    forward_loss(p, y, fwd_guard);
    if (nl == 2) {
        HIP_OK(hipEventRecord(ev_join_, s2_));
        HIP_OK(hipStreamWaitEvent(stream_, ev_join_, 0));
    }
    if (train_mode) HIP_OK(hipEventRecord(ev_loss_[loss_seq_ % LOSS_RING], stream_));
    fwd_guard.done = true;
}

// Everything that reads the fp32 masters in front of the walk, on the side stream beside the first layers: the filters' Winograd
// transforms, bf16 mirrors, quantised images and chain packing, and -- training -- the loss's l2 term; with the events the lanes wait for.
void Net::forward_filters(FwdPass& p, LossSlotGuard& guard) {
    const bool side = p.side;
    if (wino_plan_.n + wino_plan_first_.n > 0) {
        // Winograd layers (plan_winograd): the filters' transforms, fresh from the fp32 masters like the bf16 mirrors below, on the side
        // stream beside conv1_1: the first such layer's own (a launch of microseconds: what the lanes wait for), the other layers', and --
        // training -- the flipped forms of the data gradients, which only backward waits for (backward_begin)
        prof_.layer = "filters";
        hipStream_t fs = side ? hstream_ : stream_;
        wino_filter_plan(wino_plan_first_, true, false, fs);
        if (side) HIP_OK(hipEventRecord(ev_wino_first_, fs));
        wino_filter_plan(wino_plan_, true, false, fs);
        if (side) HIP_OK(hipEventRecord(ev_wino_, fs));
        if (p.train_mode && wino_plan_flip_.n > 0) {
            wino_filter_plan(wino_plan_flip_, false, true, fs);
            if (side) HIP_OK(hipEventRecord(ev_wino_flip_, fs));
            wino_flip_pending_ = side;
        }
        if (side) p.lane[0].wino_pending = p.lane[1].wino_pending = 2;
    }
    if (bf16_) {
        // the fp32 masters may have been updated by the optimizer, a variable load or the caller (external
        // arena): refresh both bf16 filter mirrors, one launch -- on the side stream, beside conv1_1 (which reads
        // the fp32 master itself); the first layer that reads a mirror waits for it
        prof_.layer = "filters";
        cast_filters(cast_plan_, params_, wq_io_, wq_oi_, side ? hstream_ : stream_);
        // ... and the quantised filter images with their scales, under the same rule (one more launch)
        if (p.run8) quantize_filters_q(quant_, quant_plan_, params_, w8_, sw8_, wsc6_, side ? hstream_ : stream_);
        if (chain_first_ >= 0) pack_tail_filters(side ? hstream_ : stream_);
        if (side) {
            HIP_OK(hipEventRecord(ev_cast_, hstream_));
            p.lane[0].cast_pending = p.lane[1].cast_pending = true;
        }
    }
    if (p.train_mode) {
        begin_loss_slot();
        guard.armed = true;
        // the l2 term reads every filter once (105 MB): on the side stream beside the first (matrix-bound) layers
        prof_.layer = "loss";
        l2_partials(params_, nfilters_, lw_, side ? hstream_ : stream_);
        if (p.nl == 2) HIP_OK(hipEventRecord(ev_l2_, hstream_));
    }
}

// Step 1 of a forward convolution: its stream, batch range and the events in front of it.  A trunk layer runs on its lane's stream.  A
// multibox head hangs off the trunk: false = this lane issues nothing (a full-batch head belongs to the last lane).
bool Net::conv_stream(FwdPass& p, int li, const Op& op, ConvRun& r) {
    Lane& ln = p.lane[li];
    if (!(op.head >= 0 && p.side)) return true;
    // the multibox heads hang off the trunk: they run on a side stream behind their feature
    // map and fill the CUs the trunk's kernels leave idle between waves of workgroups
    if (!ln.fmap_carried[op.head]) HIP_OK(hipEventRecord(ln.ev_fmap[op.head], ln.s));
    ln.fmap_carried[op.head] = false;
    if (p.heads_full) {
        // ONE launch over the whole batch on lane 0's side stream, behind both lanes' feature maps: half the
        // launches, twice the workgroups each, and lane 1's trunk (whose own "side" stream is its main
        // stream) does not queue behind its heads
        if (li < p.nl_cur - 1) return false;
        // (after the merge: the small maps' heads alternate between the side stream and the idle second lane's)
        r.cs = (p.nl_cur == 1 && op.head >= 2 && (p.small_heads++ & 1)) ? s2_ : hstream_;
        for (int l = 0; l < p.nl_cur; ++l) HIP_OK(hipStreamWaitEvent(r.cs, p.lane[l].ev_fmap[op.head], 0));
        r.nb = p.b; r.b0 = 0;
        p.lane[0].heads_on_side = true;
    } else {
        HIP_OK(hipStreamWaitEvent(ln.h, ln.ev_fmap[op.head], 0));
        r.cs = ln.h;
        ln.heads_on_side = true;
    }
    return true;
}

// Step 2: Round 6: the Winograd form (plan_winograd).  A lane owns the tile rows of its images in the layer's full-batch
// transform V (which the weight gradient reads) and its own GEMM-result scratch.
void Net::conv_wino_scratch(const FwdPass& p, int li, int op_index, const ConvDesc& d, ConvRun& r) {
    Op& op = ops_[op_index];
    const bool own = r.cs == p.lane[li].s;
    const size_t tpi = (size_t)wino_tiles(d) / d.B;
    if (op.wino_V) {      // a training handle: this launch's rows of the layer's full-batch transform
        r.wino_V = op.wino_V + (size_t)r.b0 * tpi * d.Ci;
        r.wino_vps = (size_t)p.b * tpi * d.Ci;
        if (p.train_mode) op.wino_v_step = fwd_serial_;
    } else {              // an inference handle: the stream's own scratch
        r.wino_V = wino_vs_[own ? li : 2];
        r.wino_vps = (size_t)r.nb * tpi * d.Ci;
    }
    // training: the input transform notes the relu mask of this layer's input for its own data gradient (conv.h)
    if (p.train_mode && op.wino_bits) {
        r.wino_bits = static_cast<char*>(op.wino_bits) + (size_t)r.b0 * tpi * (d.Ci / 4) * 8;
        op.wino_bits_step = fwd_serial_;
    }
}

// Step 3: the kernel, by the handle's compute type and the layer's place in the graph.
void Net::launch_conv_fwd(const FwdPass& p, const Op& op, const ConvDesc& d, const ConvRun& r) {
    const Tensor& in = tensors_[op.in];
    const Tensor& out = tensors_[op.out];
    hipStream_t cs = r.cs;
    const float* xin = reinterpret_cast<const float*>(at(in, r.b0));
    void* yout = at(out, r.b0);
    if (op.pool_after >= 0) {
        // Pool fusion (round 5): this conv's epilogue takes the 2x2 maxima itself and writes the POOLED tensor (+ the
        // pool's 12-bit record in training); its own output has no other reader -- forward or backward -- and is
        // never written (plan_pool_fusion)
        const Op& pl = ops_[op.pool_after];
        const Tensor& pt = tensors_[pl.out];
        void* rec = (pl.pool_rec && p.train_mode)
                        ? static_cast<char*>(pl.pool_rec) + (size_t)r.b0 * pt.H * pt.W * (pt.C / 4) * sizeof(unsigned short) : nullptr;
        if (r.wino_M)
            wino_fwd(d, xin, op.wino_U, params_ + op.b_off, nullptr, true, r.wino_V, r.wino_vps, r.wino_M,
                     reinterpret_cast<float*>(at(pt, r.b0)), rec, cs, r.wino_bits);
        else if (!bf16_)
            conv_fwd_pool(d, xin, params_ + op.w_off, params_ + op.b_off, reinterpret_cast<float*>(at(pt, r.b0)), rec, cs);
        else
            conv_fwd_pool_bf16(d, reinterpret_cast<const bf16_t*>(xin), wq_oi_ + op.w_off, params_ + op.b_off,
                               reinterpret_cast<bf16_t*>(at(pt, r.b0)), rec, cs);
        if (p.run8 && pt.data8)      // the pooled tensor feeds a quantised layer: the boundary's quantise pass
            quantize_q(quant_, pt, at(pt, r.b0), r.nb, q_at(pt, r.b0), cs);
        return;
    }
    if (r.wino_M)
        wino_fwd(d, xin, op.wino_U, params_ + op.b_off, static_cast<float*>(yout), op.relu, r.wino_V, r.wino_vps, r.wino_M,
                 nullptr, nullptr, cs, r.wino_bits);
    else if (!bf16_)
        conv_fwd(d, xin, params_ + op.w_off, params_ + op.b_off, static_cast<float*>(yout), op.relu, cs);
    else if (in.data_f32 && first_layer_kernel(d))      // conv1_1: fp32 image and master filter in, bf16 out
        conv_first_fwd_bf16(d, xin, params_ + op.w_off, params_ + op.b_off, static_cast<bf16_t*>(yout), op.relu, cs);
    else if (in.data_f32)
        conv_fwd_smallc_bf16out(d, xin, params_ + op.w_off, params_ + op.b_off, static_cast<bf16_t*>(yout), op.relu, cs);
    else if (p.run8 && op.fp8)
        conv_fwd_q(quant_, d, q_at(in, r.b0), w8_ + op.w8_off, sw8_ ? sw8_ + op.sw_off : nullptr, wsc6_ ? wsc6_ + op.sw_off : nullptr,
                   params_ + op.b_off, yout, q_at(out, r.b0), out.wants16, op.relu, cs);
    else
        conv_fwd_bf16(d, reinterpret_cast<const bf16_t*>(xin), wq_oi_ + op.w_off, params_ + op.b_off, yout, out.data_f32, op.relu, cs);
    // a bf16 layer in front of a quantised one: a boundary with a quantise pass of its own
    if (p.run8 && out.data8 && !op.fp8) quantize_q(quant_, out, yout, r.nb, q_at(out, r.b0), cs);
}

// One convolution on one lane.
void Net::forward_conv(FwdPass& p, int li, int op_index) {
    const Op& op = ops_[op_index];
    const Tensor& in = tensors_[op.in];
    Lane& ln = p.lane[li];
    // ---- 1. stream and events
    ConvRun r{ln.s, ln.b0, ln.nb};
    if (!conv_stream(p, li, op, r)) return;
    const ConvDesc d = conv_desc(op, r.nb);
    struct LanesScope {      // (tile choice of the bf16 kernel-row gather: the lanes share the chip's workgroup slots)
        LanesScope(int n) { g_conv_lanes = n; }
        ~LanesScope() { g_conv_lanes = 1; }
    } lanes_scope(r.nb == ln.nb ? p.nl_cur : 1);
    if (ln.cast_pending && !in.data_f32) {
        HIP_OK(hipStreamWaitEvent(ln.s, ev_cast_, 0));
        ln.cast_pending = false;
    }
    // (GEMM-result scratch: one per stream that runs such layers -- the lanes' main streams and the side stream of the heads)
    r.wino_M = !op.wino_f ? nullptr : r.cs == ln.s ? wino_m_[li] : r.cs == hstream_ ? wino_m_[2] : nullptr;
    if (r.wino_M && r.cs == ln.s && ln.wino_pending) {      // (the side stream ran the filter transforms itself)
        // (waiting for ALL transforms incl. the flipped ones before the first layer: 24.00 against 23.69 ms median,
        // profiles/r06_bc_ab_filter_split_f32.txt)
        HIP_OK(hipStreamWaitEvent(ln.s, ln.wino_pending == 2 ? ev_wino_first_ : ev_wino_, 0));
        --ln.wino_pending;
    }
    // ---- 2. Winograd scratch
    if (r.wino_M) conv_wino_scratch(p, li, op_index, d, r);
    // ---- 3. the kernel
    if (op.pool_after >= 0) {
        launch_conv_fwd(p, op, d, r);
        return;
    }
    // a feature map's producer carries the event its head waits for (common.h g_stop_event; backward_conv does the same)
    int fh = -1;      // the head that reads this op's output
    if (p.side && op.head < 0 && r.cs == ln.s)
        for (const Op& o : ops_)
            if (o.kind == OP_CONV && o.head >= 0 && o.in == op.out) { fh = o.head; break; }
    if (fh >= 0) g_stop_event = ln.ev_fmap[fh];
    struct CarryScope {
        bool* flag;
        ~CarryScope() { if (flag) *flag = g_stop_event == nullptr; g_stop_event = nullptr; }
    } carry_scope{fh >= 0 ? &ln.fmap_carried[fh] : nullptr};
    launch_conv_fwd(p, op, d, r);
}

void Net::forward_pool(FwdPass& p, int li, int op_index) {
    const Op& op = ops_[op_index];
    const Tensor& in = tensors_[op.in];
    const Tensor& out = tensors_[op.out];
    const Lane& ln = p.lane[li];
    if (op.fused_fwd) return;      // written by its producer's epilogue
    PoolDesc d{ln.nb, in.H, in.W, in.C, out.H, out.W, op.k, op.stride, op.pad_h, op.pad_w};
    if (op.pool_rec && p.train_mode) {
        void* rec = static_cast<char*>(op.pool_rec) + (size_t)ln.b0 * out.H * out.W * (in.C / 4) * sizeof(unsigned short);
        if (bf16_) maxpool_fwd_rec(d, reinterpret_cast<const bf16_t*>(at(in, ln.b0)), reinterpret_cast<bf16_t*>(at(out, ln.b0)), rec, ln.s);
        else maxpool_fwd_rec(d, reinterpret_cast<const float*>(at(in, ln.b0)), reinterpret_cast<float*>(at(out, ln.b0)), rec, ln.s);
    } else if (p.train_mode && pool_ws_ && maxpool_arg_applicable(d)) {
        // mod_pool5: the windows' first-maximum taps stay in pool_ws_ (this pool is its only user) for backward
        void* arg = static_cast<char*>(pool_ws_) + (size_t)ln.b0 * out.H * out.W * (in.C / 4) * sizeof(unsigned);
        if (bf16_) maxpool_fwd_arg(d, reinterpret_cast<const bf16_t*>(at(in, ln.b0)), reinterpret_cast<bf16_t*>(at(out, ln.b0)), arg, ln.s);
        else maxpool_fwd_arg(d, reinterpret_cast<const float*>(at(in, ln.b0)), reinterpret_cast<float*>(at(out, ln.b0)), arg, ln.s);
        pool_arg_op_ = op_index;
    } else if (p.run8 && op.fp8) {      // on the codes; bf16 as well where someone reads that
        maxpool_fwd_q(quant_, d, q_at(in, ln.b0), q_at(out, ln.b0), ln.s);
        if (out.wants16) maxpool_fwd(d, reinterpret_cast<const bf16_t*>(at(in, ln.b0)), reinterpret_cast<bf16_t*>(at(out, ln.b0)), ln.s);
    } else if (bf16_) {
        maxpool_fwd(d, reinterpret_cast<const bf16_t*>(at(in, ln.b0)), reinterpret_cast<bf16_t*>(at(out, ln.b0)), ln.s);
        if (p.run8 && out.data8)      // a bf16 pool in front of a quantised layer
            quantize_q(quant_, out, at(out, ln.b0), ln.nb, q_at(out, ln.b0), ln.s);
    } else maxpool_fwd(d, reinterpret_cast<const float*>(at(in, ln.b0)), reinterpret_cast<float*>(at(out, ln.b0)), ln.s);
}

void Net::forward_l2norm(FwdPass& p, int li, int op_index) {
    const Op& op = ops_[op_index];
    const Tensor& in = tensors_[op.in];
    const Tensor& out = tensors_[op.out];
    const Lane& ln = p.lane[li];
    if (bf16_) l2norm_fwd(ln.nb * in.H * in.W, in.C, reinterpret_cast<const bf16_t*>(at(in, ln.b0)), params_ + scale_off_,
                          reinterpret_cast<bf16_t*>(at(out, ln.b0)), ln.s);
    else l2norm_fwd(ln.nb * in.H * in.W, in.C, reinterpret_cast<const float*>(at(in, ln.b0)), params_ + scale_off_,
                    reinterpret_cast<float*>(at(out, ln.b0)), ln.s);
}

// The loss (training) or result pass behind the heads: one full-batch launch, or one per lane.
void Net::forward_loss(FwdPass& p, const float* y, LossSlotGuard& guard) {
    const int b = p.b;
    const bool train_mode = p.train_mode;
    prof_.layer = "loss";
    const int A = preset_->num_anchors, nv = C_ + 5;
    if (train_mode) { bw_loss_kind_ = loss_kind_; bw_gamma_ = focal_gamma_; bw_alpha_ = focal_alpha_; bw_loc_ = loc_; }      // the step's loss: backward follows it
    const bool focal = train_mode && bw_loss_kind_ == 1;
    // The lanes' loss launches share a self-resetting completion ticket (ops.hip): if a launch fails after another
    // lane's has been enqueued, the count never reaches the step's total and the ticket would stay non-zero for the life
    // of the handle -- drain the device and clear it before the error leaves.
    try {
    if (p.heads_full) {      // full-batch heads: one loss / result launch on the main stream behind the side stream and lane 1
        HIP_OK(hipEventRecord(ev_h_, hstream_));
        HIP_OK(hipStreamWaitEvent(stream_, ev_h_, 0));
        HIP_OK(hipEventRecord(ev_join_, s2_));
        HIP_OK(hipStreamWaitEvent(stream_, ev_join_, 0));
        if (focal) multibox_focal_loss(heads_, b, 0, b, result_, y, lw_, wd_, loss_bnorm_, bw_gamma_, bw_alpha_, stream_, bw_loc_);
        else if (train_mode) multibox_loss(heads_, b, 0, b, result_, y, lw_, wd_, loss_bnorm_, stream_, bw_loc_);
        else heads_result(heads_, b, result_, stream_);
    }
    for (int li = 0; li < p.nl && !p.heads_full; ++li) {
        Lane& ln = p.lane[li];
        if (ln.heads_on_side) {
            HIP_OK(hipEventRecord(ln.ev_h, ln.h));
            HIP_OK(hipStreamWaitEvent(ln.s, ln.ev_h, 0));
        }
        HeadLayout hl = heads_;
        for (int i = 0; i < hl.nmaps; ++i) hl.buf[i] = heads_.buf[i] + (size_t)ln.b0 * hl.hw[i] * hl.ld[i];
        float* res = result_ + (size_t)ln.b0 * A * nv;
        if (train_mode) {
            if (li == 1) HIP_OK(hipStreamWaitEvent(ln.s, ev_l2_, 0));      // the final reduction may fall to this lane
            if (focal) multibox_focal_loss(hl, ln.nb, ln.b0, b, res, y + (size_t)ln.b0 * A * nv, lw_, wd_, loss_bnorm_, bw_gamma_, bw_alpha_, ln.s, bw_loc_);
            else multibox_loss(hl, ln.nb, ln.b0, b, res, y + (size_t)ln.b0 * A * nv, lw_, wd_, loss_bnorm_, ln.s, bw_loc_);
        } else {
            heads_result(hl, ln.nb, res, ln.s);
        }
    }
    } catch (...) {
        if (train_mode && lw_.ticket) {
            (void)hipDeviceSynchronize();
            (void)hipMemset(lw_.ticket, 0, sizeof(unsigned));
        }
        guard.failed();
        throw;
    }
}

// Backward runs the op list in reverse.  It can be driven in stages so a data-parallel caller can
// start all-reducing finished gradient ranges while the rest of backward still runs: filters sit
// in the arena in forward order, so reverse execution completes them from the END of the filter
// region towards its beginning, always as one contiguous, growing suffix.
// The data-gradient chain is ONE lane (rounds 2-4 also carried a two-lane form, half batches on two sets of streams:
// fp32 -0.3 %, bf16 -7 %, profiles/r02_l_ab_bwd_lanes_*.txt -- backward already has the weight-gradient stream filling the
// data gradients' tails; removed in round 5).
void Net::launch_wgrad(int op_index, int b, hipStream_t ws, const float* ya) {
    const Op& op = ops_[op_index];
    const Tensor& in = tensors_[op.in];
    const Tensor& out = tensors_[op.out];
    const ConvDesc d = conv_desc(op, b);
    float* slab = wgrad_ws_ + op.ws_off;
    prof_.layer = op.name.c_str();
    // Round 6: from the forward's transform of the input and the transformed dy (conv.h wino_wgrad) -- if the forward pass of THIS step
    // left that transform (a launch that ran on a stream without Winograd scratch took the direct kernel: the direct weight gradient then)
    if (op.wino_w && op.wino_v_step == fwd_serial_) {
        const size_t tpi = (size_t)wino_tiles(d) / d.B;
        if (!ya) wino_bwd_transform(d, out.gf(), nullptr, wino_ya_, ws);      // (this stream's own transform: into buffer 0)
        wino_wgrad(d, op.wino_V, (size_t)b * tpi * d.Ci, ya ? ya : wino_ya_, grads_ + op.w_off, grads_ + op.b_off, params_ + op.w_off, wd_,
                   wino_slab_, ws);
        if (ws != stream_ && wino_ya2_) {      // the buffer is free again behind this GEMM: what the main stream's next write of it waits for
            const int k = ya == wino_ya2_ ? 1 : 0;
            HIP_OK(hipEventRecord(ev_ya_free_[k], ws));
            ya_free_set_[k] = true;
        }
    } else if (!bf16_) {
        conv_wgrad(d, in.f(), out.gf(), grads_ + op.w_off, grads_ + op.b_off, params_ + op.w_off, wd_, slab, ws);
    } else if (in.data_f32) {   // conv1_1
        if (first_layer_kernel(d))
            conv_first_wgrad_bf16(d, in.f(), out.gh(), grads_ + op.w_off, grads_ + op.b_off, params_ + op.w_off, wd_, slab, ws);
        else
            conv_wgrad_smallc_bf16dy(d, in.f(), out.gh(), grads_ + op.w_off, grads_ + op.b_off, params_ + op.w_off, wd_, slab, ws);
    } else {
        conv_wgrad_bf16(d, in.h(), out.gh(), grads_ + op.w_off, grads_ + op.b_off, params_ + op.w_off, wd_, slab, ws);
    }
}

// The data gradient of one convolution: into its input's gradient, or -- un-pooling (up) -- through the pool's record into the pool's
// input gradient (dst); mask: with the relu mask of the input's producer.
void Net::launch_dgrad(const Op& op, const ConvDesc& d, const Op* up, Tensor& dst, bool mask, int cls, hipStream_t ds, bool yt_done) {
    const Tensor& in = tensors_[op.in];
    const Tensor& out = tensors_[op.out];
    const bool accum = bwd_.t[op.in].done > 0;
    if (op.wino_d && cls == 0) {      // Round 6: the Winograd form (its scratch belongs to the main stream)
        if (!yt_done) wino_bwd_transform(d, out.gf(), wino_yt_, nullptr, ds);
        wino_dgrad(d, wino_yt_, op.wino_Uf, up ? dst.gf() : in.gf(), mask ? in.f() : nullptr, !up && accum, wino_xw_,
                   up ? up->pool_rec : nullptr, dst.H, dst.W, ds,
                   op.wino_bits && op.wino_bits_step == fwd_serial_ ? op.wino_bits : nullptr);      // (the forward of THIS step wrote them)
    } else if (!bf16_) {
        if (up) conv_dgrad_unpool(d, out.gf(), params_ + op.w_off, dst.gf(), up->pool_rec, dst.H, dst.W, ds);
        else conv_dgrad(d, out.gf(), params_ + op.w_off, in.gf(), mask ? in.f() : nullptr, accum, ds);
    } else {
        if (up) conv_dgrad_unpool_bf16(d, out.gh(), wq_io_ + op.w_off, dst.gh(), up->pool_rec, dst.H, dst.W, ds);
        else conv_dgrad_bf16(d, out.gh(), wq_io_ + op.w_off, in.gh(), mask ? in.h() : nullptr, accum, ds);
    }
}

// ---- Backward's cross-stream hand-offs, all of them.  M = stream_ (class 0: the data gradients of the trunk and the big heads, the
// pools, the l2-norm), S = hstream_ (class 1: the last small head and the extra layers behind conv8_1, bw_class), W = wstream_ (the
// weight gradients where overlap_ is on).  Events are recorded and waited for in host issue order; a wait takes the record that
// precedes it.  No record / wait pair of backward is written anywhere but in the functions named here.
//
//   event           recorded by, on                              waited for by, on                      what it orders
//   ev_m2s_         bw_sync(1, 0), M                             bw_sync(1, 0), S                       S reads or accumulates into a gradient M wrote
//                                                                                                       (backward_begin: the loss gradient; bw_need)
//   ev_h_           bw_sync(0, 1), S                             bw_sync(0, 1), M                       M reads or accumulates into a gradient S wrote
//                                                                                                       (conv8_1 joins the chain; the end of the pass)
//   Tensor::gev     bw_wrote, the writer's class -- or carried   bw_need, the other class               the same, for exactly the kernel that wrote it last
//                   by the kernel itself (g_stop_event)          wgrad_handoff (b), W                   W's weight gradient reads dy
//                                                                launch_tail_backward (wgrad_wait), W   the chain's grouped weight gradient reads the chain's dy
//                                                                  -- or M when the weight gradients run there and the chain ran on S
//   ev_dy_          wgrad_handoff (a), M behind the dual         wgrad_handoff (a), W                   W's GEMM reads the ya buffer the transform wrote
//                     transform
//                   wgrad_handoff (b), S or M (from_side)        wgrad_handoff (b), W                   W reads a dy that has no event of its own
//                   launch_tail_backward (wgrad_wait), the       launch_tail_backward, W or M           as Tensor::gev above, where the chain's first
//                     chain's stream                                                                    output has no event
//                   backward_join, M                             backward_join, W                       a caller that consumes the range on W finds the weight
//                                                                                                       gradients that ran on M (overlap off; conv1_1's)
//   ev_w_           backward_join, W                             backward_join, M                       the range is final in M's order: the update, the caller
//   ev_ya_free_[k]  launch_wgrad, W behind the GEMM that read    wgrad_handoff (a), M before the dual   the transform overwrites buffer k only behind its
//                     ya buffer k                                  transform that writes buffer k       last reader (write after read; outlives a pass)
//
// (backward_begin's wait for ev_wino_flip_ is forward's hand-off: the filter transforms of the data gradients, issued by forward.)
// Within a class everything is stream order.  W never writes what M or S read inside a pass: its results are the gradient arena.

// ws waits for dy's producer: for the kernel that carried the event, or for everything `from` has been given so far
void Net::wgrad_wait(hipStream_t ws, hipEvent_t carried, hipStream_t from) {
    if (carried) {
        HIP_OK(hipStreamWaitEvent(ws, carried, 0));
    } else {
        HIP_OK(hipEventRecord(ev_dy_, from));
        HIP_OK(hipStreamWaitEvent(ws, ev_dy_, 0));
    }
}

void Net::backward_begin(int b, const float* y) {
    SSD_REQUIRE(training_, "handle was created with training = 0");
    require_unswapped("backward");
    // (backward reads the flipped filter transforms and the bf16 mirrors that the LAST forward pass of any kind made from its masters)
    SSD_REQUIRE(!fwd_swapped_, "weight EMA: backward is refused behind a forward pass that ran while the average was swapped in: "
                               "run the training forward pass again");
    g_prof = &prof_;
    prof_.layer = "loss";
    const bool side = hstream_ && overlap_;
    bwd_.begin(this, b);
    if (wino_flip_pending_) {      // the data gradients' filter transforms (side stream, issued by forward)
        HIP_OK(hipStreamWaitEvent(stream_, ev_wino_flip_, 0));
        wino_flip_pending_ = false;
    }
    if (bw_loss_kind_ == 1) multibox_focal_loss_grad(heads_, b, 0, result_, y, lw_, bw_gamma_, bw_alpha_, stream_, bw_loc_);
    else multibox_loss_grad(heads_, b, 0, result_, y, lw_, stream_, bw_loc_);
    for (int t : head_t_) bw_wrote(0, t);      // the loss gradient, on the main stream
    if (side) bw_sync(1, 0);      // the side stream starts behind it (the small maps' head data gradients: bw_class)
}

// The weight gradient only feeds the optimizer; the data gradient is on the critical path.  They read the same dy and write disjoint
// buffers, so the weight gradient goes to a side stream: its workgroups fill the CUs the data-gradient's last partial wave of
// workgroups leaves idle (and vice versa).
// The first layer's weight gradient (no data gradient behind it: the main stream has gone idle by then) runs on the MAIN stream
// beside conv1_2's weight gradient instead of queueing behind it -- both are HBM-bound at half the achievable bandwidth
// (profiles/r04_a_timeline_bf16.txt: 7013 .. 7391 us of the step ran one such kernel at a time)
Net::WgradStream Net::wgrad_stream_for(bool need_dx) const {
    const bool side = wstream_ && overlap_;
    const bool on_main = side && !need_dx;
    return WgradStream{(side && !on_main) ? wstream_ : stream_, side, on_main};
}

// Makes w.ws wait for what this layer's weight gradient reads.  Returns the buffer that holds the layer's transformed dy where the
// main stream has written it (a), else nullptr.
const float* Net::wgrad_handoff(const Op& op, const ConvDesc& d, int cls, bool need_dx, const WgradStream& w) {
    // One transform of dy for both gradients (wino_bwd_transform's dual kernel: dy is read once): where the layer takes the
    // Winograd form of both, on the main stream, which the data gradient runs on.  Which layers: by shape alone, max(Ci, Co) <= 128
    // (conv1_2, conv2_x) -- there the GEMMs that run beside the transform are HBM-bound themselves and the bytes saved shorten the
    // step; on the wider layers the AT transform hides beside a compute-bound GEMM on the other stream, and moving its writes to the
    // main stream measured slower (DESIGN.md 4.9 has the rows).  wino_dual_ == 2: every such layer (the bit-identity tests).
    const bool dual = wino_dual_ && (wino_dual_ == 2 || std::max(d.Ci, d.Co) <= wino_dual_max_c_) && wino_ya2_ && need_dx && cls == 0 &&
                      op.wino_d && op.wino_w && op.wino_v_step == fwd_serial_;
    const BwdPass::Grad& dy = bwd_.t[op.out];
    if (dual) {
        // (a) the dual transform on the main stream, then ev_dy_: the weight-gradient stream waits for the transform instead of
        // dy's producer (which the main stream waits for here)
        bw_need(0, op.out);
        float* buf = bwd_.ya_turn ? wino_ya2_ : wino_ya_;
        // (the GEMM that read this buffer last, two dual layers back on the weight-gradient stream: normally long done)
        if (w.side && ya_free_set_[bwd_.ya_turn]) HIP_OK(hipStreamWaitEvent(stream_, ev_ya_free_[bwd_.ya_turn], 0));
        wino_bwd_transform(d, tensors_[op.out].gf(), wino_yt_, buf, stream_);
        if (w.side) {
            wgrad_wait(wstream_, nullptr, stream_);
            bwd_.side_used = true;
        }
        bwd_.ya_turn ^= 1;
        return buf;
    }
    if (w.side && !w.on_main) {
        // (b) the weight-gradient stream waits for the kernel that wrote dy last (it waited for the earlier writers), or for the
        // stream that holds dy.  (from_side: dy written on the main stream but already waited for by the side stream, and this op
        // lives there: the side stream is the one that is less far ahead -- a small head's weight gradient need not wait for mod_conv7)
        const bool from_side = dy.gstream == 1 || (cls == 1 && bwd_.seen[1][0] >= dy.gseq);
        wgrad_wait(wstream_, dy.gev_set ? tensors_[op.out].gev : nullptr, from_side ? hstream_ : stream_);
        bwd_.side_used = true;
        return nullptr;
    }
    // (c) the weight gradient runs on the main stream (no overlap, or the first layer's): an ordinary reader of class 0
    bw_need(0, op.out);
    if (w.on_main) bwd_.first_on_main = true;
    return nullptr;
}

// conv1_2 in bf16: the layer below is the first layer, whose only use for dx is its weight gradient -- computed here from the dx
// tiles while they are in LDS (conv.h conv_dgrad_first_wgrad_bf16); dx is never written and conv1_1's own weight-gradient kernel is
// skipped when its turn comes (backward_conv).  Returns whether the launch was taken.
bool Net::dgrad_first_wgrad(const Op& op, const ConvDesc& d, const Op* up, bool mask, int cls, hipStream_t ds) {
    if (!(fuse_first_wgrad_ && !up && mask && bwd_.t[op.in].done == 0 && cls == 0)) return false;
    if (first_conv_ < 0 || ops_[first_conv_].out != op.in) return false;      // (this op reads the first layer's output)
    const Op& f = ops_[first_conv_];
    const ConvDesc df = conv_desc(f, bwd_.b);
    if (!conv_dgrad_first_wgrad_bf16_applicable(d, df)) return false;
    prof_.layer = "conv1_2+conv1_1";
    conv_dgrad_first_wgrad_bf16(d, tensors_[op.out].gh(), wq_io_ + op.w_off, tensors_[op.in].h(), df, tensors_[input_t_].f(),
                                grads_ + f.w_off, grads_ + f.b_off, params_ + f.w_off, wd_, wgrad_ws_ + f.ws_off, ds);
    bwd_.first_fused = true;
    bwd_.fused_first_out = op.in;
    bw_wrote(cls, op.in);
    return true;
}

// One convolution: the weight gradient's stream and hand-off, its launch, then the data gradient on the op's class (bw_class): the
// small maps' heads and the chain of extra layers behind them on the side stream, everything else on the main stream.  Hand-offs
// between the two are events placed where a kernel reads or accumulates into a gradient that the other class wrote last (bw_need):
// conv8_1 joins the chain.
void Net::backward_conv(int op_index) {
    const Op& op = ops_[op_index];
    const Tensor& in = tensors_[op.in];
    const int b = bwd_.b;
    const ConvDesc d = conv_desc(op, b);
    const bool need_dx = op.in != input_t_;
    const int cls = bw_class(op, op_index);
    hipStream_t ds = cls == 1 ? hstream_ : stream_;
    const WgradStream w = wgrad_stream_for(need_dx);
    const float* ya = wgrad_handoff(op, d, cls, need_dx, w);
    if (!(bwd_.first_fused && !need_dx))      // (conv1_1's came out of conv1_2's data gradient: dgrad_first_wgrad)
        launch_wgrad(op_index, b, w.ws, ya);
    if (need_dx) {
        if (!ya) bw_need(cls, op.out);
        // Pool fusion (round 5): when this conv reads a recorded 2x2 pool's output, its data gradient routes every
        // pooled pixel's dx through the record straight into the four cells of the POOL'S INPUT gradient (relu mask of
        // that tensor's producer included, from the record's sign bit): the pooled tensor's own gradient is never
        // written and the pool's backward pass is not launched.
        const Op* up = op.unpool >= 0 ? &ops_[op.unpool] : nullptr;
        const int dst = up ? up->in : op.in;
        const int done = bwd_.t[op.in].done;
        if (!up && done > 0) bw_need(cls, op.in);      // accumulates into what the other class wrote
        const bool mask = !up && done + 1 == in.consumers && in.relu_out;
        if (!dgrad_first_wgrad(op, d, up, mask, cls, ds)) {
            g_stop_event = tensors_[dst].gev;      // the launch carries dst's event (taken by the gather launchers)
            struct Disarm { ~Disarm() { g_stop_event = nullptr; } } disarm;      // (also when the launch throws)
            launch_dgrad(op, d, up, tensors_[dst], mask, cls, ds, ya != nullptr);
            const bool carried = tensors_[dst].gev && g_stop_event == nullptr;
            bw_wrote(cls, dst, carried);
        }
    }
    bwd_.progress.retire(op_index);
}

void Net::backward_pool(int op_index) {
    const Op& op = ops_[op_index];
    if (op.fused_bwd) return;      // its consumer's data gradient has already written in.grad through the record
    const Tensor& in = tensors_[op.in];
    const Tensor& out = tensors_[op.out];
    const int done = bwd_.t[op.in].done;
    const bool last = done + 1 == in.consumers;
    bw_need(0, op.out);
    if (done > 0) bw_need(0, op.in);
    PoolDesc d{bwd_.b, in.H, in.W, in.C, out.H, out.W, op.k, op.stride, op.pad_h, op.pad_w};
    void* pws = maxpool_bwd_ws_bytes(d) ? pool_ws_ : nullptr;
    if (op.pool_rec && done == 0 && last) {      // single consumer: dx is overwritten from the forward record
        if (bf16_) maxpool_bwd_rec(d, op.pool_rec, out.gh(), in.gh(), in.relu_out, stream_);
        else maxpool_bwd_rec(d, op.pool_rec, out.gf(), in.gf(), in.relu_out, stream_);
    } else if (pool_arg_op_ == op_index && pws && maxpool_arg_applicable(d)) {      // the forward pass of this step left the record
        if (bf16_) maxpool_bwd_arg(d, in.h(), pws, out.gh(), in.gh(), done > 0, last && in.relu_out, stream_);
        else maxpool_bwd_arg(d, in.f(), pws, out.gf(), in.gf(), done > 0, last && in.relu_out, stream_);
    } else if (bf16_)
        maxpool_bwd(d, in.h(), out.gh(), in.gh(), done > 0, last && in.relu_out, pws, stream_);
    else
        maxpool_bwd(d, in.f(), out.gf(), in.gf(), done > 0, last && in.relu_out, pws, stream_);
    bw_wrote(0, op.in);
}

void Net::backward_l2norm(int op_index) {
    const Op& op = ops_[op_index];
    const Tensor& in = tensors_[op.in];
    const Tensor& out = tensors_[op.out];
    const int b = bwd_.b, cls = bw_class(op, op_index);
    hipStream_t ds = cls == 1 ? hstream_ : stream_;
    SSD_REQUIRE(bwd_.t[op.in].done == 0 && in.consumers != 1, "l2norm backward must be the first of several consumers");
    bw_need(cls, op.out);
    if (bf16_)
        l2norm_bwd(b * in.H * in.W, in.C, in.h(), params_ + scale_off_, out.gh(), in.gh(), grads_ + scale_off_, l2_ws_, ds);
    else
        l2norm_bwd(b * in.H * in.W, in.C, in.f(), params_ + scale_off_, out.gf(), in.gf(), grads_ + scale_off_, l2_ws_, ds);
    bw_wrote(cls, op.in);
}

// The joins that close a stage.
void Net::backward_join(bool finished, bool sync_main) {
    if (finished && bwd_.issued[1] > bwd_.seen[0][1]) bw_sync(0, 1);      // (every side-stream result has a main-stream reader: a no-op)
    // The returned range is final in the weight-gradient stream's order.  Make it final in
    // main-stream order too unless the caller consumes it on the weight-gradient stream itself
    // (sync_main = false keeps the data gradients running ahead); the last stage always joins.
    if (wstream_ && overlap_ && (bwd_.side_used || finished) && (sync_main || finished)) {
        HIP_OK(hipEventRecord(ev_w_, wstream_));
        HIP_OK(hipStreamWaitEvent(stream_, ev_w_, 0));
    }
    // Overlap switched off (ssd_set_overlap(0) / SSD_OVERLAP_WGRAD=0): the weight gradients ran on the main
    // stream.  A caller that consumes the range on the weight-gradient stream (sync_main = false) must still
    // find it final there, so that stream waits for the main stream instead.  The same holds for the first layer's weight
    // gradient, which is issued on the main stream (wgrad_stream_for).
    if (wstream_ && !sync_main && (!overlap_ || (finished && bwd_.first_on_main))) wgrad_wait(wstream_, nullptr, stream_);
}

// A stage: the reverse ops until the filter range that is newly final holds min_floats, then the joins.
bool Net::backward_step(size_t min_floats, size_t* off, size_t* count, bool sync_main) {
    require_unswapped("backward");
    bwd_.side_used = false;
    for (int op_index; (op_index = bwd_.progress.next(min_floats)) >= 0;) {
        const Op& op = ops_[op_index];
        const bool ablated = op_ablated(op.name, op.kind, op.head, op.k);
        prof_.layer = op.name.c_str();
        if (chain_bwd_ && in_chain_[op_index] && !ablated) {
            // Round 6 (plan_tail_chain): the first chain op met issues the chain's data gradients (one launch) and every chain layer's
            // weight gradient (one grouped launch); the other members are skipped when their turn comes -- all but the chain's first
            // layer, whose data and weight gradients are ordinary launches below (launch_tail_backward leaves it out of the group)
            if (!bwd_.progress.chain_done) {
                launch_tail_backward();      // (retires them)
                prof_.layer = op.name.c_str();
            }
            if (op_index != chain_first_) continue;
        }
        if (ablated) bwd_.progress.retire(op_index);
        else if (op.kind == OP_CONV) backward_conv(op_index);
        else if (op.kind == OP_POOL) backward_pool(op_index);
        else backward_l2norm(op_index);
        bwd_.t[op.in].done++;
    }
    const bool finished = bwd_.progress.finished();
    backward_join(finished, sync_main);
    const std::pair<size_t, size_t> range = bwd_.progress.end_stage();
    *off = range.first;
    *count = range.second;
    return !finished;
}

std::vector<std::pair<size_t, size_t>> Net::backward_ranges(size_t min_floats) const {
    std::vector<std::pair<size_t, size_t>> out;
    BwProgress p;
    p.begin(this);
    while (!p.finished()) {
        for (int i; (i = p.next(min_floats)) >= 0;) p.retire(i);
        const std::pair<size_t, size_t> range = p.end_stage();
        if (range.second > 0) out.push_back(range);
    }
    return out;
}

void Net::set_wgrad_stream(hipStream_t s) {
    SSD_REQUIRE(training_, "handle was created with training = 0");
    hip_.free_stream(wstream_);      // (the handle's own: the hardware queues go by which streams exist)
    wstream_ = s;
    s2_ = s;      // a training handle's second forward lane lives on the weight-gradient stream
}

void Net::backward(int b, const float* y) {
    backward_begin(b, y);
    size_t off, count;
    while (backward_step(nparams_, &off, &count, true)) {}
}

float Net::current_lr() const {
    for (size_t i = 0; i < lr_bounds_.size(); ++i)
        if (global_step <= lr_bounds_[i]) return lr_values_[i];
    return lr_values_[lr_bounds_.size()];
}

void Net::apply_gradients(float grad_scale) {
    SSD_REQUIRE(training_, "handle was created with training = 0");
    require_unswapped("the update");
    g_prof = &prof_;
    prof_.layer = "optimizer";
    if (rule_kind_ == UPDATE_ADAMW) ++adam_t_;      // t counts this update, skipped by the clipped kernel or not
    float* report = clip_max_norm_ != 0.f ? begin_clip_slot() : nullptr;      // where the update leaves {norm, factor}
    if (rule_kind_ == UPDATE_ADAMW)
        adamw_update(params_, mom_, adam_v_, grads_, nparams_, nfilters_, current_lr(), adam_b1_, adam_b2_, adam_eps_, adam_decay_,
                     adam_t_, grad_scale, clip_max_norm_, clip_ws_, report, stream_);
    else if (!report)
        momentum_update(params_, mom_, grads_, nparams_, current_lr(), momentum_, grad_scale, stream_);
    else
        momentum_update_clipped(params_, mom_, grads_, nparams_, current_lr(), momentum_, grad_scale, clip_max_norm_, clip_ws_, report, stream_);
    if (report) end_clip_slot();
    // the average follows every update enqueued, one that the clipped kernel skipped too: like global_step, t is a function of the
    // updates taken
    if (ema_decay_ != 0.f) {
        ema_update(ema_, params_, nparams_, ema_decay_, ema_t_, stream_);
        ++ema_t_;
    }
    ++global_step;      // a skipped update counts: the schedule is a function of the steps taken
}

void Net::require_unswapped(const char* what) const {
    SSD_REQUIRE(!ema_swapped_, "weight EMA: %s is refused while the average is swapped in (ssd_ema_swap)", what);
}

void Net::set_ema(float decay) {
    SSD_REQUIRE(training_, "weight EMA: the handle was created with training = 0");
    require_unswapped("ssd_set_ema");
    if (decay != 0.f && ema_decay_ == 0.f) {
        const size_t bytes = nparams_ * sizeof(float);
        // on first use, so that a handle that never averages holds the memory it held without the option
        if (!ema_) {
            ema_ = static_cast<float*>(hip_.mem(bytes));
            ev_ema_ = hip_.event();
        }
        HIP_OK(hipMemcpyAsync(ema_, params_, bytes, hipMemcpyDeviceToDevice, stream_));
        // a rare call: the copy is finished when it returns, so a caller who gives the handle another stream afterwards
        // (set_stream orders nothing) finds the first EMA update behind it
        HIP_OK(hipStreamSynchronize(stream_));
        ema_t_ = 0;
    }
    ema_decay_ = decay;
}

void Net::set_ema_step(long long t) {
    SSD_REQUIRE(training_, "weight EMA: the handle was created with training = 0");
    require_unswapped("ssd_set_ema_step");
    SSD_REQUIRE(t >= 0, "weight EMA: the count of EMA updates must be >= 0, got %lld", t);
    ema_t_ = t;
}

void Net::ema_swap_arenas() {
    SSD_REQUIRE(training_, "weight EMA: the handle was created with training = 0");
    SSD_REQUIRE(ema_decay_ != 0.f, "weight EMA: nothing to swap, the EMA is off (ssd_set_ema)");
    g_prof = &prof_;
    prof_.layer = "optimizer";
    // Nothing else needs refreshing: what a pass reads besides the fp32 masters -- the Winograd filter transforms, the bf16 mirrors,
    // the quantised images, the packed tail filters -- forward_filters derives from the masters at the head of every pass, and
    // backward, which reads the flipped transforms and mirrors of the last forward pass, is refused until the weights are back and
    // a forward pass has run on them (fwd_swapped_).
    // Everything a pass reads from the masters on a side stream is waited for by its lanes, but for the flipped transforms of a
    // training pass, which only backward waits for: the swap waits for them too (the wait stays pending for backward).
    if (wino_flip_pending_) HIP_OK(hipStreamWaitEvent(stream_, ev_wino_flip_, 0));
    ema_swap(params_, ema_, nparams_, stream_);
    // The side streams read the masters at the head of a pass (forward_filters), and an fp32 inference pass of fewer than 8 samples
    // does not make them wait for the main stream (forward: neither bf16_ nor train_mode nor two lanes): they wait for the swap here.
    HIP_OK(hipEventRecord(ev_ema_, stream_));
    if (hstream_) HIP_OK(hipStreamWaitEvent(hstream_, ev_ema_, 0));
    if (s2_ && s2_ != hstream_) HIP_OK(hipStreamWaitEvent(s2_, ev_ema_, 0));
    ema_swapped_ = !ema_swapped_;
}

void Net::set_grad_clip(float max_norm) {
    SSD_REQUIRE(training_, "gradient clipping: the handle was created with training = 0");
    clip_max_norm_ = max_norm;
}

void Net::set_update_rule(int kind, float b1, float b2, float eps, float decay) {
    SSD_REQUIRE(training_, "update rule: the handle was created with training = 0");
    const size_t bytes = nparams_ * sizeof(float);
    if (kind == UPDATE_ADAMW && !adam_v_) {
        // on first use, so that a handle that stays under momentum holds the memory it held without the rule
        adam_v_ = static_cast<float*>(hip_.mem(bytes));
        HIP_OK(hipMemsetAsync(adam_v_, 0, bytes, stream_));
    }
    if (kind != rule_kind_) {
        // the accumulators mean different things under the two rules
        HIP_OK(hipMemsetAsync(mom_, 0, bytes, stream_));
        if (adam_v_) HIP_OK(hipMemsetAsync(adam_v_, 0, bytes, stream_));
        adam_t_ = 0;
    }
    rule_kind_ = kind;
    adam_b1_ = b1; adam_b2_ = b2; adam_eps_ = eps; adam_decay_ = decay;
}

void Net::get_update_rule(int* kind, float* b1, float* b2, float* eps, float* decay) const {
    *kind = rule_kind_;
    *b1 = adam_b1_; *b2 = adam_b2_; *eps = adam_eps_; *decay = adam_decay_;
}

void Net::set_adam_step(long long t) {
    SSD_REQUIRE(training_, "update rule: the handle was created with training = 0");
    SSD_REQUIRE(t >= 0, "update rule: the count of AdamW updates must be >= 0, got %lld", t);
    adam_t_ = t;
}

void Net::get_grad_norm_step(int steps_back, float out[2]) {
    SSD_REQUIRE(training_, "gradient clipping: the handle was created with training = 0");
    SSD_REQUIRE(steps_back >= 0 && steps_back < LOSS_RING - 1, "steps_back must be in 0..%d", LOSS_RING - 2);
    SSD_REQUIRE(clip_max_norm_ != 0.f, "gradient clipping is off: no update has measured a gradient norm (ssd_set_grad_clip)");
    SSD_REQUIRE(clip_seq_ - steps_back >= 0, "gradient clipping: no clipped update has run %d update(s) back", steps_back);
    const int slot = (int)((clip_seq_ - steps_back) % LOSS_RING);
    HIP_OK(hipEventSynchronize(ev_clip_[slot]));
    out[0] = clip_host_[2 * slot];
    out[1] = clip_host_[2 * slot + 1];
}

// backward + update of a single-GPU step.  (Rounds 2-4 carried an "early update" of the finished arena suffix on the
// weight-gradient stream: +-0.1 %, profiles/r02_h -- backward ends with conv1_1's weight gradient alone on that stream, both
// are HBM-bound, there is nothing for the update to hide behind.  Removed in round 5.)
void Net::backward_apply(int b, const float* y, float grad_scale) {
    SSD_REQUIRE(training_, "handle was created with training = 0");
    backward(b, y);
    apply_gradients(grad_scale);
}

void Net::null_gradients_step() {
    SSD_REQUIRE(training_, "handle was created with training = 0");
    require_unswapped("a step without samples");      // (its gradient is the L2 term of the raw weights)
    null_gradients(params_, grads_, nfilters_, nparams_, wd_, stream_);
    // a step without samples has no loss kernel: its slot of the ring is written here, after the slot's previous user
    // (LOSS_RING passes ago) has finished -- no kernel in flight writes to it
    float* slot = begin_loss_slot();
    for (int i = 0; i < 4; ++i) slot[i] = 0.f;
    HIP_OK(hipEventRecord(ev_loss_[loss_seq_ % LOSS_RING], stream_));
}

void Net::set_optimizer(const float* lr_values, const long long* bounds, int n, float momentum, float wd) {
    SSD_REQUIRE(n >= 1, "need at least one learning rate value");
    lr_values_.assign(lr_values, lr_values + n);
    lr_bounds_.assign(bounds, bounds + (n - 1));
    momentum_ = momentum;
    wd_ = wd;
}

void Net::upload_xy(const float* x, const float* y, int b) {
    SSD_REQUIRE(b >= 1 && b <= Bmax_, "batch %d outside 1..%d (max_batch)", b, Bmax_);
    const size_t nx = (size_t)b * preset_->image_h * preset_->image_w * 3;
    HIP_OK(hipMemcpyAsync(x_stage_, x, nx * sizeof(float), hipMemcpyHostToDevice, stream_));
    if (y) {
        const size_t ny = (size_t)b * preset_->num_anchors * (C_ + 5);
        HIP_OK(hipMemcpyAsync(y_stage_, y, ny * sizeof(float), hipMemcpyHostToDevice, stream_));
    }
}

// The clip ring, like the losses': the slot's previous update (LOSS_RING updates ago) has long finished; nothing here waits for this one
float* Net::begin_clip_slot() {
    ++clip_seq_;
    const int slot = (int)(clip_seq_ % LOSS_RING);
    if (clip_seq_ >= LOSS_RING) HIP_OK(hipEventSynchronize(ev_clip_[slot]));
    return clip_dev_ + 2 * slot;
}

void Net::end_clip_slot() { HIP_OK(hipEventRecord(ev_clip_[clip_seq_ % LOSS_RING], stream_)); }

float* Net::begin_loss_slot() {
    ++loss_seq_;
    const int slot = (int)(loss_seq_ % LOSS_RING);
    if (loss_seq_ >= LOSS_RING) HIP_OK(hipEventSynchronize(ev_loss_[slot]));      // its previous pass (long finished)
    lw_.losses = losses_dev_ + 4 * slot;
    return losses_host_ + 4 * slot;
}

void Net::get_losses(float out[4]) {
    HIP_OK(hipStreamSynchronize(stream_));
    const int slot = loss_seq_ < 0 ? 0 : (int)(loss_seq_ % LOSS_RING);
    for (int i = 0; i < 4; ++i) out[i] = losses_host_[4 * slot + i];
}

void Net::get_losses_step(int steps_back, float out[4]) {
    SSD_REQUIRE(steps_back >= 0 && steps_back < LOSS_RING - 1, "steps_back must be in 0..%d", LOSS_RING - 2);
    SSD_REQUIRE(loss_seq_ - steps_back >= 0, "no step with a loss has run %d step(s) back", steps_back);
    const int slot = (int)((loss_seq_ - steps_back) % LOSS_RING);
    HIP_OK(hipEventSynchronize(ev_loss_[slot]));
    for (int i = 0; i < 4; ++i) out[i] = losses_host_[4 * slot + i];
}

void Net::set_result(const float* pred_dev, int b) {
    SSD_REQUIRE(b >= 1 && b <= Bmax_, "batch %d outside 1..%d", b, Bmax_);
    HIP_OK(hipMemcpyAsync(result_, pred_dev, (size_t)b * preset_->num_anchors * (C_ + 5) * sizeof(float), hipMemcpyDeviceToDevice, stream_));
}

void Net::copy_result(float* out, int b) {
    const size_t n = (size_t)b * preset_->num_anchors * (C_ + 5);
    HIP_OK(hipMemcpyAsync(out, result_, n * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_OK(hipStreamSynchronize(stream_));
}

// ---------------------------------------------------------------------------------
// variables
// ---------------------------------------------------------------------------------
const Variable& Net::find_var(const char* name) const {
    for (const Variable& v : vars_)
        if (v.name == name) return v;
    fail("no such variable: %s", name ? name : "(null)");
    return vars_[0];
}

void Net::load_variable(const char* name, const float* host, size_t count, int which) {
    const Variable& v = find_var(name);
    SSD_REQUIRE(count == v.count(), "variable %s holds %zu floats, got %zu", name, v.count(), count);
    SSD_REQUIRE(which != 3 || adam_v_, "second moment of %s: the handle has never been under AdamW (ssd_set_update_rule)", name);
    SSD_REQUIRE(which != 4 || ema_, "weight EMA of %s: the handle has never been under a weight EMA (ssd_set_ema)", name);
    if (which == 0 || which == 4) require_unswapped(which == 0 ? "ssd_load_variable" : "ssd_load_ema");
    float* base = which == 0 ? params_ : which == 3 ? adam_v_ : which == 4 ? ema_ : mom_;
    SSD_REQUIRE(base != nullptr, "arena not allocated (training = 0?)");
    HIP_OK(hipStreamSynchronize(stream_));
    HIP_OK(hipMemcpy2D(base + v.off, v.pitch * sizeof(float), host, v.width * sizeof(float), v.width * sizeof(float), v.rows,
                       hipMemcpyHostToDevice));
}

void Net::save_variable(const char* name, float* host, size_t count, int which) {
    const Variable& v = find_var(name);
    SSD_REQUIRE(count == v.count(), "variable %s holds %zu floats, got %zu", name, v.count(), count);
    SSD_REQUIRE(which != 3 || adam_v_, "second moment of %s: the handle has never been under AdamW (ssd_set_update_rule)", name);
    SSD_REQUIRE(which != 4 || ema_, "weight EMA of %s: the handle has never been under a weight EMA (ssd_set_ema)", name);
    const float* base = which == 0 ? params_ : (which == 1 ? grads_ : which == 3 ? adam_v_ : which == 4 ? ema_ : mom_);
    SSD_REQUIRE(base != nullptr, "arena not allocated (training = 0?)");
    HIP_OK(hipStreamSynchronize(stream_));
    HIP_OK(hipMemcpy2D(host, v.width * sizeof(float), base + v.off, v.pitch * sizeof(float), v.width * sizeof(float), v.rows,
                       hipMemcpyDeviceToHost));
}

void Net::activation_shape(const char* name, int* H, int* W, int* C) const {
    if (name && (!strncmp(name, "grad:", 5) || !strncmp(name, "bf16:", 5))) name += 5;
    const bool want_scale = name && !strncmp(name, "scale:", 6);      // (mxfp8 handle: one value per pixel and 32 channels)
    if (want_scale) name += 6;
    for (const Tensor& t : tensors_)
        if (t.name == name) {
            *H = t.H; *W = t.W; *C = want_scale ? t.C / 32 : t.C;
            return;
        }
    fail("no such activation: %s", name ? name : "(null)");
}

void Net::activation(const char* name, int b, float* out, size_t count) {
    // "grad:<scope>" returns d(loss)/d(pre-activation) of that layer from the last backward
    // "bf16:<scope>" (fp8 handle) returns the bf16 form of a tensor that is also kept as e4m3 (the default for such a tensor
    // is its dequantised e4m3 form)
    const bool want_grad = name && !strncmp(name, "grad:", 5);
    if (want_grad) name += 5;
    const bool want_bf16 = name && !strncmp(name, "bf16:", 5);
    if (want_bf16) name += 5;
    // "scale:<scope>" (mxfp8 handle) returns the block scales 2^x of an MX tensor, [b, H, W, C / 32]
    const bool want_scale = name && !want_grad && !want_bf16 && !strncmp(name, "scale:", 6);
    if (want_scale) name += 6;
    for (size_t ti = 0; ti < tensors_.size(); ++ti) {
        const Tensor& t = tensors_[ti];
        if (t.name != name || !t.data) continue;
        SSD_REQUIRE(!want_grad || t.grad != nullptr, "no gradient storage (training = 0?)");
        SSD_REQUIRE(!(want_grad && bwd_.first_fused && bwd_.fused_first_out == (int)ti),
                    "gradient of %s is not materialised: the first layer's weight gradient was computed inside the next layer's data gradient (SSD_POOL_FUSE=3 keeps it)", name);
        for (const Op& op : ops_) {
            SSD_REQUIRE(!(op.kind == OP_POOL && op.fused_fwd && op.in == (int)ti && !want_grad),
                        "activation %s is not materialised: its 2x2 pool is fused into the convolution (SSD_POOL_FUSE=0 keeps it)", name);
            SSD_REQUIRE(!(op.kind == OP_POOL && op.fused_bwd && op.out == (int)ti && want_grad),
                        "gradient of %s is not materialised: the pool's backward is fused into its consumer's data gradient (SSD_POOL_FUSE=0 keeps it)", name);
        }
        if (want_scale) {
            SSD_REQUIRE(t.scale8 != nullptr, "activation %s has no block scales (not an MX tensor of an mxfp8 handle)", name);
            const size_t want = quant_scale_bytes(quant_, t.per_image()) * b;
            SSD_REQUIRE(count == want, "scale:%s holds %zu floats for b=%d, got %zu", name, want, b, count);
            HIP_OK(hipStreamSynchronize(stream_));
            std::vector<unsigned char> hs(count);
            HIP_OK(hipMemcpy(hs.data(), t.scale8, count, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < count; ++i) out[i] = ldexpf(1.f, (int)hs[i] - 127);
            return;
        }
        SSD_REQUIRE(count == t.per_image() * b, "activation %s holds %zu floats for b=%d, got %zu", name, t.per_image() * b, b,
                    count);
        const void* src = want_grad ? t.grad : t.data;
        HIP_OK(hipStreamSynchronize(stream_));
        if (t.data8 && !want_grad && !want_bf16) {      // a quantised tensor: its dequantised codes
            std::vector<unsigned char> hc(quant_code_bytes(quant_, count)), hs(quant_scale_bytes(quant_, count));
            HIP_OK(hipMemcpy(hc.data(), t.data8, hc.size(), hipMemcpyDeviceToHost));
            if (!hs.empty()) HIP_OK(hipMemcpy(hs.data(), t.scale8, hs.size(), hipMemcpyDeviceToHost));
            dequantize_host(quant_, hc.data(), hs.empty() ? nullptr : hs.data(), t.scale, count, out);
            return;
        }
        SSD_REQUIRE(!(quant_ != Quant::none && !want_grad && !t.wants16), "activation %s of the fp8 handle has no bf16 form", name);
        if (want_grad ? t.grad_f32 : t.data_f32) {
            HIP_OK(hipMemcpy(out, src, count * sizeof(float), hipMemcpyDeviceToHost));
        } else {        // bf16 storage: widen on the host (exact)
            std::vector<unsigned short> hb(count);
            HIP_OK(hipMemcpy(hb.data(), src, count * 2, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < count; ++i) {
                const unsigned u = (unsigned)hb[i] << 16;
                memcpy(out + i, &u, 4);
            }
        }
        return;
    }
    fail("no such activation: %s", name ? name : "(null)");
}

// ---------------------------------------------------------------------------------
// decode + NMS of the last result
// ---------------------------------------------------------------------------------
// Two output slots alternate, each one packed buffer [count | conf | cls | idx | box] in pinned, device-mapped
// host memory: the kernels are enqueued, an event marks their end, and the caller collects a slot later
// (detect_fetch) -- e.g. after it has launched the next batch -- or at once.
static size_t det_count_bytes(int b) { return ((size_t)b * 4 + 255) / 256 * 256; }

void Net::detect_slot_carve(const DetectSlot& sl, DetectOut& d, char* base) const {
    const size_t n = (size_t)sl.b * sl.out_cap;
    d.count = (int*)base;
    d.conf = (float*)(base + det_count_bytes(sl.b));
    d.cls = (int*)(d.conf + n);
    d.idx = d.cls + n;
    d.box = d.idx + n;
}

DetectSlot& Net::detect_slot_next(int b, int out_cap) {
    det_cur_ ^= 1;
    DetectSlot& sl = det_slot_[det_cur_];
    if (!sl.ready) {
        sl.ready = hip_.event();
    } else {
        HIP_OK(hipEventSynchronize(sl.ready));      // the slot's previous copy must have landed before it is reused
    }
    // The survivors (a few hundred KB per batch, only count-many entries per image are written) go STRAIGHT into pinned,
    // device-mapped host memory from the per-image kernel's ordered emit -- like the four losses (alloc()): a
    // device-to-host copy of the whole [b][out_cap] arrays is a blit KERNEL of its own behind the pass (13 us per batch of
    // 128 in the rocprofv3 trace, a third of the pass) plus one more launch for the host to issue.
    const size_t need = det_count_bytes(b) + (size_t)b * out_cap * 28;
    if (need > sl.bytes) {
        if (sl.host) hip_.free_pinned(sl.host);
        sl.dev = sl.host = nullptr;
        sl.bytes = 0;
        const size_t grow = std::max(need, det_count_bytes(Bmax_) + (size_t)Bmax_ * std::min(out_cap, 200) * 28);
        void* dp = nullptr;
        sl.host = static_cast<char*>(hip_.pinned(grow, &dp));
        sl.dev = static_cast<char*>(dp);
        sl.bytes = grow;
    }
    sl.b = b; sl.out_cap = out_cap; sl.used = need;
    return sl;
}

const DetectSlot& Net::detect_last_dev(int b, float thr, int cap, int max_out, int out_cap, bool nms, DetectOut* dev_out) {
    SSD_REQUIRE(b >= 1 && b <= Bmax_, "batch %d outside 1..%d", b, Bmax_);
    SSD_REQUIRE(out_cap >= 1, "out_cap must be >= 1");
    const int A = preset_->num_anchors;
    if (!detect_ws_) {
        detect_ws_ = hip_.mem(detect_ws_bytes(Bmax_, A));
    }
    DetectSlot& sl = detect_slot_next(b, out_cap);
    g_prof = &prof_;
    prof_.layer = "detect";
    DetectOut d;
    detect_slot_carve(sl, d, sl.dev);
    detect(A, C_, anchors_dev_, result_, b, thr, cap, max_out, out_cap, nms, d, detect_ws_, stream_);
    HIP_OK(hipEventRecord(sl.ready, stream_));
    if (dev_out) *dev_out = d;
    return sl;
}

const DetectSlot& Net::detect_last_all_dev(int b, float thr, int nms_top_k, int keep_top_k, int out_cap, DetectOut* dev_out,
                                           const NmsParams& nms) {
    nms_params_check("detect_last_all", &nms);
    SSD_REQUIRE(b >= 1 && b <= Bmax_, "batch %d outside 1..%d", b, Bmax_);
    const int A = preset_->num_anchors;
    detection_output_check(A, C_, b, thr, nms_top_k, keep_top_k, out_cap);      // before a slot is taken
    const size_t need = detection_output_ws_bytes(Bmax_, C_, nms_top_k);
    if (need > detout_ws_bytes_) {
        if (detout_ws_) hip_.free_mem(detout_ws_);      // (waits for the device)
        detout_ws_ = nullptr;
        detout_ws_bytes_ = 0;
        detout_ws_ = hip_.mem(need);
        detout_ws_bytes_ = need;
    }
    DetectSlot& sl = detect_slot_next(b, out_cap);
    g_prof = &prof_;
    prof_.layer = "detect";
    DetectOut d;
    detect_slot_carve(sl, d, sl.dev);
    detection_output(A, C_, anchors_dev_, result_, b, thr, nms_top_k, keep_top_k, out_cap, d, detout_ws_, detout_ws_bytes_, stream_,
                     nms);
    HIP_OK(hipEventRecord(sl.ready, stream_));
    if (dev_out) *dev_out = d;
    return sl;
}

void Net::detect_fetch(int which, int* count, float* conf, int* cls, int* idx, int* box) {
    SSD_REQUIRE(which == 0 || which == 1, "which must be 0 (latest) or 1 (the one before)");
    DetectSlot& sl = det_slot_[det_cur_ ^ which];
    SSD_REQUIRE(sl.ready != nullptr && sl.b > 0, "no detection pass in that slot");
    HIP_OK(hipEventSynchronize(sl.ready));
    DetectOut h;
    detect_slot_carve(sl, h, sl.host);
    const size_t n = (size_t)sl.b * sl.out_cap;
    if (count) memcpy(count, h.count, (size_t)sl.b * 4);
    if (conf) memcpy(conf, h.conf, n * 4);
    if (cls) memcpy(cls, h.cls, n * 4);
    if (idx) memcpy(idx, h.idx, n * 4);
    if (box) memcpy(box, h.box, n * 16);
}

void Net::detect_host(int which, DetectOut* host, int* b, int* out_cap) {
    SSD_REQUIRE(which == 0 || which == 1, "which must be 0 (latest) or 1 (the one before)");
    SSD_REQUIRE(host != nullptr, "null argument");
    DetectSlot& sl = det_slot_[det_cur_ ^ which];
    SSD_REQUIRE(sl.ready != nullptr && sl.b > 0, "no detection pass in that slot");
    HIP_OK(hipEventSynchronize(sl.ready));
    detect_slot_carve(sl, *host, sl.host);
    if (b) *b = sl.b;
    if (out_cap) *out_cap = sl.out_cap;
}

void Net::detect_last(int b, float thr, int cap, int max_out, int out_cap, bool nms, int* count, float* conf, int* cls,
                      int* idx, int* box) {
    detect_last_dev(b, thr, cap, max_out, out_cap, nms, nullptr);
    detect_fetch(0, count, conf, cls, idx, box);
}

}  // namespace ssd
