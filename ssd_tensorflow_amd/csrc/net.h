// The SSD-VGG step executor: layer table, HBM arenas, forward / backward schedules.
// Mirrors the graph SSDVGG.build_from_vgg assembles (ssdvgg.py:96-118, 190-372) and the
// loss/optimizer of build_optimizer (ssdvgg.py:375-599).
#pragma once
#include "common.h"
#include "conv.h"
#include "ops.h"
#include "boxes.h"
#include "bf16.h"
#include "quant_layout.h"
#include <string>
#include <vector>
#include <map>

namespace ssd {

struct Tensor {
    std::string name;        // TF scope of the producing op ("conv4_3", "pool3", "norm_conv4_3", "head2")
    int H = 0, W = 0, C = 0;
    bool relu_out = false;   // produced by conv+relu: gradients written into it get the relu mask
    int consumers = 0;       // ops reading it in forward
    hipEvent_t gev = nullptr;    // optional: recorded behind every kernel that writes grad, so a reader on the other class waits for
                                 // THAT kernel instead of everything its class has been given (what a pass knows of it: Net::BwdPass)
    bool data_f32 = true;    // storage of data: fp32, or bf16 (bf16 configuration, every tensor but the image and the head outputs)
    bool grad_f32 = true;    // storage of grad
    void* data = nullptr;
    void* grad = nullptr;
    // quantised handle (net.hip plan_fp8): the tensor's code image for its quantised readers, in the handle's format (quant_layout.h;
    // a sample of it: Net::q_at), and its scale (fp8); wants16: it also has a reader that takes the bf16 form
    unsigned char* data8 = nullptr;
    float scale = 0.f;
    // MX kinds: the E8M0 block scales of data8, written by the tensor's producer
    unsigned char* scale8 = nullptr;
    bool wants16 = true;
    size_t per_image() const { return (size_t)H * W * C; }
    const float* f() const { return static_cast<const float*>(data); }
    float* gf() const { return static_cast<float*>(grad); }
    const bf16_t* h() const { return static_cast<const bf16_t*>(data); }
    bf16_t* gh() const { return static_cast<bf16_t*>(grad); }
};

enum OpKind { OP_CONV, OP_POOL, OP_L2NORM };

struct Op {
    OpKind kind;
    std::string name;        // TF variable scope for conv ops
    int in = -1, out = -1;   // tensor ids
    // conv
    int KH = 1, KW = 1, stride = 1, dil = 1, pad_h = 0, pad_w = 0;
    bool relu = true;
    size_t w_off = 0, b_off = 0;     // offsets (floats) into the arenas
    size_t ws_off = 0;               // this layer's region of the weight-gradient slab workspace (floats)
    // pool
    int k = 2;
    void* pool_rec = nullptr;        // forward-written argmax / sign record of a single-consumer 2x2 pool (ops.h)
    // pool fusion (net.hip plan_pool_fusion): a pool written by its producer's forward epilogue / whose backward is the scatter
    // in its consumer's data gradient; on conv ops: the pool behind this conv / the pool this conv's data gradient un-pools
    bool fused_fwd = false, fused_bwd = false;
    int pool_after = -1, unpool = -1;
    // head op: index of the feature map, else -1
    int head = -1;
    // fp8 handle (net.hip plan_fp8): a convolution that runs on conv_fwd_fp8 or conv_bigk_fwd_fp8 / a pool that runs on e4m3 bytes; sw_off = the
    // layer's per-channel filter scales
    bool fp8 = false;
    size_t sw_off = 0;
    size_t w8_off = 0;      // byte offset of the layer's code image in w8_ (fp8, mxfp8: its arena offset w_off; mxfp6: packed, three quarters the size)
    // Round 6 (fp32): the Winograd F(4x4, 3x3) form of this layer's passes (net.hip plan_winograd; conv.h wino_*): forward, data
    // gradient, weight gradient; the layer's filter transforms [36][Ci][Co] / [36][Co][Ci] and its input's transform [36][tiles][Ci]
    // (written by forward, read by the weight gradient)
    bool wino_f = false, wino_d = false, wino_w = false;
    float *wino_U = nullptr, *wino_Uf = nullptr, *wino_V = nullptr;
    void* wino_bits = nullptr;       // the relu mask of the layer's input as bits (forward's input transform -> the data gradient's output transform)
    long long wino_bits_step = -1;   // the forward pass that wrote them (Net::fwd_serial_)
    long long wino_v_step = -1;      // the forward pass that wrote wino_V
};

struct Variable {
    std::string name;        // reference TF variable name
    int ndim;
    int shape[4];
    // location inside the arena: `rows` rows of `width` floats, `pitch` apart, from `off`
    size_t off, rows, width, pitch;
    size_t count() const { return rows * width; }
};

// one output slot of the decode + NMS pass: packed [count | conf | cls | idx | box] in pinned, device-mapped host memory
struct DetectSlot {
    char* dev = nullptr;            // the device's view of `host` (no HBM copy, no transfer)
    char* host = nullptr;
    size_t bytes = 0, used = 0;
    int b = 0, out_cap = 0;
    hipEvent_t ready = nullptr;     // recorded behind the pass
};

class Net {
public:
    // dtype 0: fp32 everywhere (BASELINE.json configs[1]); 1: bf16 activations / gradients / filter mirrors with fp32
    // master weights, fp32 accumulation and fp32 loss (configs[2]); 2: fp8, an inference-only bf16 handle whose eligible
    // trunk convolutions (conv3_2 ... mod_conv7) run on e4m3 operands (plan_fp8); 3: mxfp8, the same layers with E8M0 block scales
    // chosen by each producer (conv_mxfp8.hip): no per-tensor scales, no calibration; 4: mxfp6, the mxfp8 plan on e2m3 operands
    // with block scales on activations and filters (conv_mxfp6.hip), layers with more than 9 taps on bf16
    Net(const char* preset, int num_classes, int max_batch, int device, bool training, unsigned long long seed,
        float* ext_params, float* ext_grads, float* ext_momentum, int dtype = 0, int graph = 0);
    ~Net();

    // graph 0: the a-trous graph (ssdvgg.py __build_vgg_mods_a_trous: 3x3 dilation-6 mod_conv6 and 1x1 mod_conv7, 1024 wide);
    // 1: the fc graph (ssdvgg.py __build_vgg_mods: VGG-16's fc6 / fc7 as a 7x7 and a 1x1 convolution, 4096 wide, variables fc6/* and fc7/*)
    static size_t arena_floats(const char* preset, int num_classes, int graph = 0);

    void set_stream(hipStream_t s) { stream_ = s; }
    hipStream_t stream() const { return stream_; }

    // steps; x/y device pointers
    void forward(const float* x, int b, bool train_mode, const float* y);
    void backward(int b, const float* y);
    void backward_begin(int b, const float* y);
    // runs reverse ops until >= min_floats of filter gradients are newly final; [off, off+count) is that range
    bool backward_step(size_t min_floats, size_t* off, size_t* count, bool sync_main);
    // the (offset, count) ranges backward_step(min_floats, ...) reports, in order, without running anything: a rank whose
    // shard is empty issues the collectives of the ranks that do run backward (parallel.train_step_dp)
    std::vector<std::pair<size_t, size_t>> backward_ranges(size_t min_floats) const;
    void set_wgrad_stream(hipStream_t s);      // caller-owned side stream for the weight gradients
    void apply_gradients(float grad_scale);
    void backward_apply(int b, const float* y, float grad_scale);      // backward + update, the optimizer overlapped with backward's tail
    void set_loss_normalizer(float bnorm) { loss_bnorm_ = bnorm; }      // <= 0: every step's own batch size
    // which loss the steps compute from the next forward on: 0 mining (the default), 1 focal with (gamma, alpha)
    void set_loss(int kind, float gamma, float alpha) { loss_kind_ = kind; focal_gamma_ = gamma; focal_alpha_ = alpha; }
    void get_loss(int* kind, float* gamma, float* alpha) const { *kind = loss_kind_; *gamma = focal_gamma_; *alpha = focal_alpha_; }
    // ... and which localization loss: 0 smooth-L1 (the default; weight 1), 1 GIoU with its weight
    void set_loc_loss(int kind, float weight) { loc_.kind = kind; loc_.weight = weight; }
    void get_loc_loss(int* kind, float* weight) const { *kind = loc_.kind; *weight = loc_.weight; }
    // clip the gradient by its global norm from the next update on: 0 off (the plain update's launch), > 0 the threshold,
    // +inf measures and never clips (ops.h momentum_update_clipped); the caller has checked the value
    void set_grad_clip(float max_norm);
    float grad_clip() const { return clip_max_norm_; }
    // {norm, factor} of the last clipped update (steps_back = 0) or of one of the LOSS_RING - 2 before it: waits for THAT update only
    void get_grad_norm_step(int steps_back, float out[2]);
    // which rule apply_gradients runs from the next update on: 0 momentum (the default), 1 AdamW with its four hyper-parameters
    // (ops.h adamw_update); the caller has checked the values.  A DIFFERENT kind zeroes the accumulators and the count of AdamW
    // updates on the handle's stream; the same kind keeps them.  The second moment is allocated on the first switch to AdamW.
    void set_update_rule(int kind, float b1, float b2, float eps, float decay);
    void get_update_rule(int* kind, float* b1, float* b2, float* eps, float* decay) const;
    long long adam_step() const { return adam_t_; }      // AdamW updates enqueued since the state was zeroed (skipped ones count)
    void set_adam_step(long long t);
    // the weight EMA (include/ssdvgg_hip.h "weight EMA"; ops.h ema_update): decay in (0, 1) switches it on -- the arena allocated
    // on the first enabling, filled with the parameters and t = 0 on every switch from off to on -- and 0 off; the caller has
    // checked the value.  While it is on, one EMA update follows every update apply_gradients enqueues.
    void set_ema(float decay);
    float ema_decay() const { return ema_decay_; }
    long long ema_step() const { return ema_t_; }        // EMA updates enqueued since the last enabling
    void set_ema_step(long long t);
    bool ema_swapped() const { return ema_swapped_; }
    // the contents of the parameter arena and the EMA arena exchanged (one kernel on the handle's stream): the next forward derives
    // every mirror and transform from the masters afresh.  While swapped, updates, backward and loads into either arena are refused.
    void ema_swap_arenas();
    void null_gradients_step();                                        // gradient arena of a step without samples
    void set_optimizer(const float* lr_values, const long long* bounds, int n, float momentum, float wd);

    // host-buffer conveniences
    void upload_xy(const float* x, const float* y, int b);
    const float* x_stage() const { return x_stage_; }
    const float* y_stage() const { return y_stage_; }

    void get_losses(float out[4]);                       // the last step's; waits for everything on the stream
    // the losses of the last step (steps_back = 0) or of one of the LOSS_RING - 1 steps before it: waits for THAT step's
    // forward only, so a caller can book step k - 1 while step k runs (train.py)
    void get_losses_step(int steps_back, float out[4]);
    void copy_result(float* out, int b);
    void set_result(const float* pred_dev, int b);

    const std::vector<Variable>& variables() const { return vars_; }
    void load_variable(const char* name, const float* host, size_t count, int which);   // 0 params, 2 momentum, 3 second moment, 4 EMA
    void save_variable(const char* name, float* host, size_t count, int which);         // 0 params, 1 grads, 2 momentum, 3 second moment, 4 EMA
    void activation(const char* name, int b, float* out, size_t count);
    void activation_shape(const char* name, int* H, int* W, int* C) const;
    void pool_fusion(int* out, int cap, int* count) const;      // per 2x2 stride-2 pool in graph order: bit 0 fused forward, bit 1 fused backward

    void detect_last(int b, float thr, int cap, int max_out, int out_cap, bool nms, int* count, float* conf, int* cls, int* idx, int* box);
    // asynchronous form: the kernels enqueued; dev_out (optional) = the device's view of the slot's arrays
    const DetectSlot& detect_last_dev(int b, float thr, int cap, int max_out, int out_cap, bool nms, DetectOut* dev_out);
    // the DetectionOutput pass (boxes.h detection_output) on the last result, into the same two alternating slots
    const DetectSlot& detect_last_all_dev(int b, float thr, int nms_top_k, int keep_top_k, int out_cap, DetectOut* dev_out,
                                          const NmsParams& nms = NmsParams{NMS_HARD, 0.f, 0.f, 0.f});
    // host copy of the latest (which = 0) or the previous (which = 1) pass; waits for that slot's pass only
    void detect_fetch(int which, int* count, float* conf, int* cls, int* idx, int* box);
    // the pinned host memory of that slot itself (valid until the second-next pass); waits for the slot's pass only
    void detect_host(int which, DetectOut* host, int* b, int* out_cap);

    const Preset& preset() const { return *preset_; }
    int num_classes() const { return C_; }
    int nvars() const { return C_ + 5; }
    int max_batch() const { return Bmax_; }
    bool training() const { return training_; }
    int dtype() const { return quant_ == Quant::fp8 ? 2 : quant_ == Quant::mxfp8 ? 3 : quant_ == Quant::mxfp6 ? 4 : bf16_ ? 1 : 0; }
    // fp8 handle: one scale per tensor that a convolution writes as e4m3, in graph order
    void fp8_calibrate(const float* x_dev, int b, bool accumulate);      // the graph on the bf16 kernels; scale = max(absmax, tiny) / 448
    int fp8_num_scales() const;
    const char* fp8_scale_name(int i) const;
    void fp8_get_scales(float* out, int n) const;
    void fp8_set_scales(const float* v, int n);
    int graph() const { return fc_ ? 1 : 0; }
    int device() const { return device_; }
    float* params() { return params_; }
    float* grads() { return grads_; }
    float* momentum() { return mom_; }
    size_t nparams() const { return nparams_; }
    size_t nfilters() const { return nfilters_; }
    float* result() { return result_; }
    long long global_step = 0;
    Profiler& profiler() { return prof_; }
    void set_overlap(bool on) { overlap_ = on; }
    void set_wino_dual(int mode) { wino_dual_ = mode; }      // backward transforms a Winograd layer's dy once for both gradients (wgrad_handoff)

private:
    int add_tensor(const std::string& name, int H, int W, int C, bool relu_out);
    void build_graph();
    void alloc();
    void init_weights(unsigned long long seed);
    ConvDesc conv_desc(const Op& op, int b) const;
    float current_lr() const;
    const Variable& find_var(const char* name) const;

    const Preset* preset_;
    int C_, Bmax_, device_;
    bool training_;
    bool bf16_ = false;
    bool fc_ = false;                      // the fc graph (arena_floats)
    // The quantised format of an inference handle's eligible layers (dtype 2 ... 4; bf16_ is set too), quant_layout.h.  fp8 and mxfp8:
    // e4m3 filter images [tap][Co][Ci] in w8_ at the filters' arena offsets + per-channel scales in sw8_, refreshed from the fp32
    // masters by every forward pass like the bf16 mirrors (one launch, behind cast_filters).  mxfp6 (conv_mxfp6.hip): the filter
    // images lie in w8_ at Op::w8_off with their block scales in wsc6_ at Op::sw_off (bytes), and layers with more than 9 taps stay on bf16
    Quant quant_ = Quant::none;
    unsigned char* wsc6_ = nullptr;
    QView q_at(const Tensor& t, int b0) const;      // sample b0 of t's quantised form
    bool fp8_calibrated_ = false, fp8_as_bf16_ = false;      // fp8_as_bf16_: this pass is the calibration run
    unsigned char* w8_ = nullptr;
    float *sw8_ = nullptr, *absmax8_ = nullptr;
    FilterQuantPlan quant_plan_;
    std::vector<int> fp8_scaled_;          // the tensors that own a scale (pool outputs share their input's)
    void plan_fp8();
    void fp8_share_pool_scales();
    void require_fp8() const;
    bf16_t *wq_io_ = nullptr, *wq_oi_ = nullptr;     // bf16 mirrors of the filter region: [tap][Ci][Co] and [tap][Co][Ci]
    FilterCastPlan cast_plan_;
    hipStream_t stream_ = nullptr;
    hipStream_t wstream_ = nullptr;        // side stream of the weight gradients (SSD_OVERLAP_WGRAD=0 disables)
    hipEvent_t ev_dy_ = nullptr, ev_w_ = nullptr;
    hipStream_t hstream_ = nullptr;        // side stream of the multibox heads in forward
    hipEvent_t ev_h_ = nullptr, ev_cast_ = nullptr, ev_fmap_[MAX_MAPS] = {};
    hipStream_t s2_ = nullptr;                  // second forward lane: its main stream, which also runs its heads (= wstream_ in a training handle)
    hipEvent_t ev2_h_ = nullptr, ev_l2_ = nullptr, ev_join_ = nullptr, ev2_fmap_[MAX_MAPS] = {};
    int tail_first_ = 0;                 // op index of conv8_1: the extra layers behind it form backward's side chain
    // Issue orders (net.hip build_orders): forward walks fwd_order_ (every multibox head right behind its feature map), backward
    // walks bwd_order_ (reverse graph order)
    std::vector<int> fwd_order_, bwd_order_;
    // Which filter ranges have their final gradient.  backward_step retires every convolution it has issued, backward_ranges walks
    // bwd_order_ with an instance of its own and launches nothing: both report their stages from the same loop condition (next)
    // and the same chain rule (retire).
    struct BwProgress {
        const Net* net = nullptr;
        std::vector<char> done;          // conv ops retired so far (indexed like ops_)
        bool chain_done = false;         // the tail chain's members (all but chain_first_) are retired: they finish together
        int pos = 0;                     // next entry of bwd_order_
        size_t hi = 0, lo = 0;           // the current stage's range so far: [lo, hi)
        void begin(const Net* n);
        int next(size_t min_floats);     // the stage's next op, -1 once it has gathered min_floats or the order is exhausted
        bool finished() const;
        size_t retire(int op_index);     // -> lo; a chain member met first retires the chain with it
        void retire_chain();             // launch_tail_backward, behind the chain's grouped weight-gradient launch
        std::pair<size_t, size_t> end_stage();      // (offset, count) of the stage; the next one starts below it
    private:
        size_t final_lo() const;         // lowest arena offset such that every filter at or above it has its final gradient
    };
    // The state of one backward pass, the counterpart of FwdPass.  It lives in the handle because a pass spans backward_begin and
    // several backward_step calls; backward_begin resets all of it (begin), nothing else does.
    // Stream classes: 0 = the main stream, 1 = the side stream (bw_class).  issued[c] counts the kernels class c has been given that
    // write a gradient, seen[x][y] is the count of class y that class x has already been made to wait for.
    struct BwdPass {
        struct Grad {                    // what the pass knows of one tensor's gradient
            int done = 0;                // consumers whose data gradient has been issued
            int gstream = 0;             // stream class of the last kernel that wrote it ...
            long gseq = 0;               // ... and that kernel's number in the class' issue order (bw_need)
            bool gev_set = false;        // Tensor::gev stands behind that kernel
        };
        int b = 0;
        BwProgress progress;
        long issued[2] = {0, 0}, seen[2][2] = {{0, 0}, {0, 0}};
        bool first_on_main = false;      // the first layer's weight gradient was issued on the main stream (wgrad_handoff)
        bool first_fused = false;        // it was computed inside the next layer's data gradient instead (dgrad_first_wgrad) ...
        int fused_first_out = -1;        // ... and this tensor's gradient (conv1_1's output) was not materialised
        int ya_turn = 1;                 // which of wino_ya_ / wino_ya2_ the next dual transform writes (wgrad_handoff)
        bool side_used = false;          // the current stage gave the weight-gradient stream work (backward_join)
        std::vector<Grad> t;             // indexed like tensors_
        void begin(const Net* n, int batch);
    } bwd_;
    hipEvent_t ev_m2s_ = nullptr;        // main -> side hand-off
    bool fuse_first_wgrad_ = false;      // bf16: conv1_1's weight gradient inside conv1_2's data gradient where the kernel applies (plan_pool_fusion)
    int first_conv_ = -1;                // op index of the convolution that reads the image (plan_pool_fusion)
    // ya: the layer's transformed dy where the main stream's dual transform has already written it (wgrad_handoff), else nullptr
    void launch_wgrad(int op_index, int b, hipStream_t ws, const float* ya = nullptr);
    // the data gradient of one convolution into dst (= in, or the input of the pool `up` it un-pools), on ds
    // (yt_done: wino_yt_ already holds this layer's transformed dy)
    void launch_dgrad(const Op& op, const ConvDesc& d, const Op* up, Tensor& dst, bool mask, int cls, hipStream_t ds, bool yt_done = false);
    // A backward pass (net.hip, "Backward"): backward_step is the stage loop, the chain and ablation skips and backward_join; the
    // members below do the rest.  Every cross-stream hand-off of backward goes through one of bw_sync / bw_need / bw_wrote,
    // wgrad_handoff (and its primitive wgrad_wait), backward_join and launch_wgrad's release of a ya buffer.
    struct WgradStream { hipStream_t ws; bool side, on_main; };
    void backward_conv(int op_index);
    WgradStream wgrad_stream_for(bool need_dx) const;
    const float* wgrad_handoff(const Op& op, const ConvDesc& d, int cls, bool need_dx, const WgradStream& w);
    void wgrad_wait(hipStream_t ws, hipEvent_t carried, hipStream_t from);
    bool dgrad_first_wgrad(const Op& op, const ConvDesc& d, const Op* up, bool mask, int cls, hipStream_t ds);
    void backward_pool(int op_index);
    void backward_l2norm(int op_index);
    void backward_join(bool finished, bool sync_main);
    // Round 6 (bf16): the latency-bound tail as one launch per direction (conv.h TailStage; net.hip plan_tail_chain).  chain_first_ =
    // op index of the first 1x1 layer below the 10x10 map (vgg300: conv9_1, vgg512: conv10_1), -1: off; in_chain_[op] marks the
    // extra layers from there on and the multibox heads that read them.
    int chain_first_ = -1;
    std::vector<char> in_chain_;
    bf16_t* wq_tail_ = nullptr;                          // the chain layers' filters in the chain kernel's fragment order (conv.h tail_chain_pack_filters) ...
    std::vector<long long> tail_fwd_off_, tail_bwd_off_; // ... element offsets per op of the forward / data-gradient form (-1: none)
    void pack_tail_filters(hipStream_t s);               // from the fresh bf16 mirrors, one launch (forward, behind cast_filters)
    bool chain_fwd_ = false, chain_bwd_ = false;      // SSD_TAIL_FUSE bit 0 / bit 1: the chain in forward / in backward
    void plan_tail_chain();
    // Round 6 (fp32): Winograd layers.  Scratch shared by every such layer: the GEMM results of a forward lane (wino_m_), the
    // transformed dy / dx of the data gradient (main stream: wino_yt_, wino_xw_), the transformed dy and the slabs of the weight
    // gradient (weight-gradient stream: wino_ya_, wino_slab_).  One stream runs each kind in order, so one buffer per kind suffices --
    // but for the transformed dy of the weight gradient where the MAIN stream writes it (wino_dual_: one transform of dy for both
    // gradients, wgrad_handoff): two buffers taken in turn (wino_ya_, wino_ya2_), so that the transform of one layer does not wait for
    // the weight-gradient stream's GEMM of the layer before.  ev_ya_free_[k]: the last GEMM that read buffer k, recorded on the
    // weight-gradient stream; the main stream waits for it before it writes the buffer again.
    void plan_winograd();
    long long fwd_serial_ = 0;           // forward passes so far
    WinoFilterPlan wino_plan_, wino_plan_first_, wino_plan_flip_;      // forward transforms of all layers but the first / of the first / flipped ones
    bool wino_flip_pending_ = false;
    bool wino_any_f_ = false, wino_any_d_ = false;
    float *wino_m_[3] = {nullptr, nullptr, nullptr}, *wino_vs_[3] = {nullptr, nullptr, nullptr}, *wino_yt_ = nullptr, *wino_xw_ = nullptr, *wino_ya_ = nullptr, *wino_slab_ = nullptr;
    hipEvent_t ev_wino_ = nullptr, ev_wino_first_ = nullptr, ev_wino_flip_ = nullptr;
    float* wino_ya2_ = nullptr;
    hipEvent_t ev_ya_free_[2] = {nullptr, nullptr};
    bool ya_free_set_[2] = {false, false};
    int wino_dual_ = 1;                  // 0 off, 1 the layers of the shape rule (wino_dual_max_c_), 2 every layer with both gradients in this form
    int wino_dual_max_c_ = 128;          // the rule: max(Ci, Co) <= this (SSD_WINO_DUAL_MAX_C): where the GEMMs beside the transform are HBM-bound themselves
    // A forward pass (net.hip, "steps"): forward builds the lanes, walks fwd_order_ and joins; the members below do the rest.
    struct Lane {
        hipStream_t s, h;
        hipEvent_t* ev_fmap;
        hipEvent_t ev_h;
        int b0, nb;
        bool heads_on_side, cast_pending;
        int wino_pending;                 // filter-transform events this lane has still to wait for: 2 = the first layer's, then 1 = the rest
        bool fmap_carried[MAX_MAPS];      // the feature map's producer carried ev_fmap[head] itself (g_stop_event)
    };
    struct FwdPass {                      // the state of one pass, on forward's stack
        Lane lane[2];
        int nl, nl_cur;                   // lanes of the pass / of the current op (they merge at conv8_1)
        bool heads_full;                  // with two lanes the multibox heads run as full-batch launches (forward_conv)
        int small_heads;
        int b;
        bool train_mode, run8, side;      // run8: the quantised layers run on their codes (the calibration pass does not)
    };
    struct LossSlotGuard;
    struct ConvRun;
    void forward_filters(FwdPass& p, LossSlotGuard& guard);
    void forward_conv(FwdPass& p, int li, int op_index);
    bool conv_stream(FwdPass& p, int li, const Op& op, ConvRun& r);
    void conv_wino_scratch(const FwdPass& p, int li, int op_index, const ConvDesc& d, ConvRun& r);
    void launch_conv_fwd(const FwdPass& p, const Op& op, const ConvDesc& d, const ConvRun& r);
    void forward_pool(FwdPass& p, int li, int op_index);
    void forward_l2norm(FwdPass& p, int li, int op_index);
    void forward_loss(FwdPass& p, const float* y, LossSlotGuard& guard);
    void launch_tail_forward(int b0, int nb, hipStream_t s);
    void launch_tail_backward();
    void build_orders();
    void plan_pool_fusion();
    int bw_class(const Op& op, int op_index) const;
    void bw_sync(int x, int y);          // class x waits for everything class y has been given so far
    void bw_need(int x, int ti);         // class x is about to read or accumulate into tensor ti's gradient
    void bw_wrote(int x, int ti, bool carried = false);      // class x has been given the kernel that writes it
    bool overlap_ = true;

    std::vector<Tensor> tensors_;
    std::vector<Op> ops_;
    std::vector<Variable> vars_;
    int input_t_ = -1;
    std::vector<int> head_t_;             // head output tensors per map
    HeadLayout heads_{};

    size_t nparams_ = 0, nfilters_ = 0, scale_off_ = 0;
    float *params_ = nullptr, *grads_ = nullptr, *mom_ = nullptr;

    float* result_ = nullptr;
    float *x_stage_ = nullptr, *y_stage_ = nullptr;
    float* wgrad_ws_ = nullptr;
    float* l2_ws_ = nullptr;
    void* pool_ws_ = nullptr;
    int pool_arg_op_ = -1;               // the 3x3 stride-1 pool whose first-maximum taps the last training forward left in pool_ws_
    void* loss_ws_ = nullptr;
    LossWork lw_{};
    static constexpr int LOSS_RING = 4;
    float* losses_host_ = nullptr;        // pinned, device-mapped: LOSS_RING slots of 4 floats, slot = loss_seq_ % LOSS_RING
    float* losses_dev_ = nullptr;         // the device's view of the same memory
    hipEvent_t ev_loss_[LOSS_RING] = {};  // recorded behind the forward pass that wrote the slot
    long long loss_seq_ = -1;             // forward passes with a loss so far - 1
    float* begin_loss_slot();             // next slot: waits until its previous use (LOSS_RING passes ago) has finished
    // gradient clipping (apply_gradients): 0 off, > 0 the threshold, +inf measure only.  The norm and the factor of every clipped
    // update land in a ring like the losses', keyed by the count of such updates, an event behind each update.
    float clip_max_norm_ = 0.f;
    void* clip_ws_ = nullptr;             // grad_norm_ws_bytes(nparams_): allocated with the arenas
    float* clip_host_ = nullptr;          // pinned, device-mapped: LOSS_RING slots of 2 floats
    float* clip_dev_ = nullptr;
    hipEvent_t ev_clip_[LOSS_RING] = {};
    long long clip_seq_ = -1;             // clipped (or measured) updates so far - 1
    float* begin_clip_slot();             // next slot (the device's view): waits until its previous use (LOSS_RING updates ago) has finished
    void end_clip_slot();                 // records the slot's event behind the update
    // the update rule (apply_gradients): under AdamW mom_ is the first moment and adam_v_ the second
    int rule_kind_ = 0;                   // UPDATE_MOMENTUM / UPDATE_ADAMW (ops.h)
    float adam_b1_ = 0.9f, adam_b2_ = 0.999f, adam_eps_ = 1e-8f, adam_decay_ = 0.01f;
    long long adam_t_ = 0;
    float* adam_v_ = nullptr;             // nparams_ floats from hip_, null until the handle is first put under AdamW
    // the weight EMA (apply_gradients, behind the update)
    float* ema_ = nullptr;                // nparams_ floats from hip_, null until the EMA is first switched on
    float ema_decay_ = 0.f;               // 0: off
    long long ema_t_ = 0;
    bool ema_swapped_ = false;            // the parameter arena holds the average and ema_ the raw weights (ema_swap_arenas)
    bool fwd_swapped_ = false;            // ema_swapped_ at the last forward pass: what its mirrors and filter transforms were made from
    hipEvent_t ev_ema_ = nullptr;         // behind every swap: the side streams wait for it (made with ema_)
    void require_unswapped(const char* what) const;
    double* anchors_dev_ = nullptr;
    int* anchors_abs_dev_ = nullptr;
    void* detect_ws_ = nullptr;
    void* detout_ws_ = nullptr;     // DetectionOutput's workspace: grown on first use, freed with the handle
    size_t detout_ws_bytes_ = 0;
    DetectSlot& detect_slot_next(int b, int out_cap);      // the other slot, free for a new pass of b x out_cap
    DetectSlot det_slot_[2];
    int det_cur_ = 0;
    void detect_slot_carve(const DetectSlot& sl, DetectOut& d, char* base) const;

    std::vector<float> lr_values_{0.001f};
    std::vector<long long> lr_bounds_;
    float momentum_ = 0.9f, wd_ = 0.0005f;
    float loss_bnorm_ = 0.f;
    int loss_kind_ = 0;                     // SSD_LOSS_MINING / SSD_LOSS_FOCAL
    int bw_loss_kind_ = 0;                  // the kind the last training forward computed: its backward takes the same
    float focal_gamma_ = 2.f, focal_alpha_ = 0.25f, bw_gamma_ = 2.f, bw_alpha_ = 0.25f;
    LocLoss loc_{}, bw_loc_{};              // SSD_LOC_SMOOTH_L1 / SSD_LOC_GIOU and its weight; bw_: of the last training forward
    Profiler prof_;
    // Every buffer, pinned page, event and stream above that the handle made itself.  Declared after every member that holds its
    // handles, so it is destroyed before them: the device is synchronised before the members above (prof_'s events) go.
    HipOwner hip_;
    TailTables tail_tables_{hip_, {}};   // the tail chain's stage tables (one per direction and lane start) in hip_'s memory
};

}  // namespace ssd
