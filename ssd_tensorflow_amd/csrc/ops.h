// HBM-bound layers around the convolutions: pooling, L2 normalisation, the multibox
// head assembly + loss, the optimizer.  Host interface (all pointers are device memory).
#pragma once
#include "common.h"

namespace ssd {

// ---- max pooling, NHWC, TF SAME semantics (padded cells never win) ---------------
// Replaces the SavedModel's pool1-4 and tf.nn.max_pool at ssdvgg.py:234-236.
struct PoolDesc {
    int B, Hi, Wi, C, Ho, Wo, k, stride, pad_h, pad_w;
};
struct bf16_t;      // bf16.h; every tensor-typed op below exists for fp32 and for bf16 storage (fp32 math)
void maxpool_fwd(const PoolDesc& d, const float* x, float* y, hipStream_t s);
void maxpool_fwd(const PoolDesc& d, const bf16_t* x, bf16_t* y, hipStream_t s);
// dx[cell] = sum of dy over the windows whose FIRST maximum (scan order) is this cell.
// accumulate: += existing dx first; relu_mask: zero where x <= 0 (x is a relu output).
// ws: optional scratch of maxpool_bwd_ws_bytes() for overlapping windows (per-window argmax bytes);
// nullptr = recompute every window's maximum per cell.
size_t maxpool_bwd_ws_bytes(const PoolDesc& d);
void maxpool_bwd(const PoolDesc& d, const float* x, const float* dy, float* dx, bool accumulate, bool relu_mask,
                 void* ws, hipStream_t s);
void maxpool_bwd(const PoolDesc& d, const bf16_t* x, const bf16_t* dy, bf16_t* dx, bool accumulate, bool relu_mask,
                 void* ws, hipStream_t s);

// 3x3 stride-1 pooling whose forward pass keeps the windows' first-maximum taps in `arg` (maxpool_bwd_ws_bytes): backward from that
// record is maxpool_bwd's second pass alone
bool maxpool_arg_applicable(const PoolDesc& d);
void maxpool_fwd_arg(const PoolDesc& d, const float* x, float* y, void* arg, hipStream_t s);
void maxpool_fwd_arg(const PoolDesc& d, const bf16_t* x, bf16_t* y, void* arg, hipStream_t s);
void maxpool_bwd_arg(const PoolDesc& d, const float* x, const void* arg, const float* dy, float* dx, bool accumulate, bool relu_mask, hipStream_t s);
void maxpool_bwd_arg(const PoolDesc& d, const bf16_t* x, const void* arg, const bf16_t* dy, bf16_t* dx, bool accumulate, bool relu_mask, hipStream_t s);

// 2x2 stride-2 pooling with a forward-written record (per window and channel: first maximum's cell + "maximum is
// positive"): backward = record + dy -> dx without re-reading the pooled tensor.  For a pooled tensor with a single
// consumer (dx is overwritten, not accumulated); relu_mask as above.
bool maxpool_rec_applicable(const PoolDesc& d);
size_t maxpool_rec_bytes(const PoolDesc& d);
void maxpool_fwd_rec(const PoolDesc& d, const float* x, float* y, void* rec, hipStream_t s);
void maxpool_fwd_rec(const PoolDesc& d, const bf16_t* x, bf16_t* y, void* rec, hipStream_t s);
void maxpool_bwd_rec(const PoolDesc& d, const void* rec, const float* dy, float* dx, bool relu_mask, hipStream_t s);
void maxpool_bwd_rec(const PoolDesc& d, const void* rec, const bf16_t* dy, bf16_t* dx, bool relu_mask, hipStream_t s);

// ---- l2_normalization (ssdvgg.py:80-84): y = scale * x * rsqrt(max(sum_c x^2, 1e-12))
void l2norm_fwd(int npix, int C, const float* x, const float* scale, float* y, hipStream_t s);
void l2norm_fwd(int npix, int C, const bf16_t* x, const float* scale, bf16_t* y, hipStream_t s);
size_t l2norm_bwd_ws_floats(int npix, int C);
void l2norm_bwd(int npix, int C, const float* x, const float* scale, const float* dy, float* dx, float* dscale,
                float* ws, hipStream_t s);
void l2norm_bwd(int npix, int C, const bf16_t* x, const float* scale, const bf16_t* dy, bf16_t* dx, float* dscale,
                float* ws, hipStream_t s);

// ---- multibox heads: layout + softmax + loss (ssdvgg.py:353-372, 375-580) ----------
constexpr int MAX_MAPS = 8;
struct HeadLayout {
    int nmaps, A, nvars;             // nvars = num_classes + 5
    int hw[MAX_MAPS];                // cells per map
    int nj[MAX_MAPS];                // box types per map
    int ld[MAX_MAPS];                // row stride of the fused head buffer (nj*nvars rounded up to 8)
    int off[MAX_MAPS + 1];           // first anchor of each map
    float* buf[MAX_MAPS];            // [B*hw][ld] raw fused head conv outputs
    void* dbuf[MAX_MAPS];            // same shape, gradients: fp32, or bf16 when grad_bf16
    int grad_bf16;
};
// row stride of a map's fused head buffer: its nj box types' nvars values, rounded up to 8 channels (whole 16-byte
// pieces in fp32 and in bf16 rows)
inline int head_ld(int nj, int nvars) { return (nj * nvars + 7) / 8 * 8; }
// the layout of nmaps maps of hw[i] cells and nj[i] box types: ld, off[] and A filled in, buffers null, fp32 gradients
HeadLayout head_layout(int nmaps, const int* hw, const int* nj, int nvars);
// result[b][a][:] = (softmax(logits), loc) in the reference's anchor order
// (map -> box type -> row -> col, ssdvgg.py:63,365 == ssdutils.py:104-116).
void heads_result(const HeadLayout& L, int B, float* result, hipStream_t s);

struct LossWork {                    // per-step scratch, all device
    float* ce;                       // [B][A] cross entropy
    float* sl1;                      // [B][A] localization term: smooth-L1 summed over the 4 offsets, or weight * (1 - GIoU)
    unsigned char* pos;              // [B][A] 1 = positive anchor
    unsigned char* sel;              // [B][A] 1 = contributes to the confidence loss
    float* sample;                   // [B][4]: conf_b, loc_b, weight_b (1/(pos_n*B) or 0), pos_n
    float* partial;                  // [1024] sum-of-squares partials
    float* losses;                   // [4] total, localization, confidence, l2 (the executor points this at mapped host memory)
    unsigned* ticket;                // completion ticket of the per-sample workgroups (zero between launches)
};
// The localization half of the multibox loss: kind 0 = smooth-L1 on the four encoded offsets (the reference's, the default; weight
// unused), 1 = weight * (1 - GIoU) of the box the offsets describe against the box the label offsets describe, both in units of
// their anchor.  The per-anchor term takes the place of the smooth-L1 sum in LossWork::sl1; everything after the
// head kernels is shared.  weight finite and > 0: checked by the callers.
struct LocLoss {
    int kind = 0;
    float weight = 1.f;
};
size_t loss_work_bytes(int B, int A);
void loss_work_carve(LossWork& w, void* base, int B, int A);
// Forward of the loss; labels [B][A][nvars] device.  result must hold heads_result's output.
// bnorm: the batch size the per-sample losses are averaged over (<= 0: this step's own B).  A data-parallel
// caller whose shards are unequal passes global_samples / world, so that the mean over ranks is the global mean.
// A step may compute its loss in several launches over disjoint sample ranges (forward lanes): L.buf, result and labels
// point at the range's first sample, B = samples of this launch, b_off = index of its first sample, B_total = the step's.
void multibox_loss(const HeadLayout& L, int B, int b_off, int B_total, const float* result, const float* labels, LossWork& w,
                   float weight_decay, float bnorm, hipStream_t s, LocLoss loc = {});
// sum of squares of the filter region into w.partial (the l2 term of multibox_loss, which must follow it in stream
// order): 4 bytes per parameter, independent of the forward pass, so the step runs it beside the first layers
void l2_partials(const float* filters, size_t nfilters, LossWork& w, hipStream_t s);
// d(loss)/d(head outputs) written into L.dbuf (pad columns stay zero).
// (lane form like multibox_loss: L.dbuf, result and labels point at sample b_off, B samples)
void multibox_loss_grad(const HeadLayout& L, int B, int b_off, const float* result, const float* labels, const LossWork& w,
                        hipStream_t s, LocLoss loc = {});

// The focal loss (softmax form) on the same buffers, lanes and workspace: heads_kernel<true> as above, then
// focal_sample_kernel / focal_grad_kernel.  Every anchor contributes alpha_t * (1 - p_t)^gamma * ce, a sample is normalised
// by max(pos_n, 1), sel is all ones; the gradient is dense.  gamma in [0, 5], alpha in (0, 1): checked by the callers.
void multibox_focal_loss(const HeadLayout& L, int B, int b_off, int B_total, const float* result, const float* labels, LossWork& w,
                         float weight_decay, float bnorm, float gamma, float alpha, hipStream_t s, LocLoss loc = {});
void multibox_focal_loss_grad(const HeadLayout& L, int B, int b_off, const float* result, const float* labels, const LossWork& w,
                              float gamma, float alpha, hipStream_t s, LocLoss loc = {});

// ---- MomentumOptimizer without Nesterov (ssdvgg.py:586-588): acc = m*acc + g; w -= lr*acc
void momentum_update(float* w, float* acc, const float* g, size_t n, float lr, float momentum, float gscale,
                     hipStream_t s);
// ... with the gradient clipped by its global norm (include/ssdvgg_hip.h "gradient clipping").  max_norm == 0: the
// call above.  Otherwise three launches on s and no host wait: grad_norm_kernel (one fp64 partial sum of squares per block),
// grad_norm_finish_kernel (one block: the partials in a fixed tree, then norm, factor and the update's scale into ws and, where
// report != NULL, norm and factor into report[0..1] -- device or device-mapped host memory), momentum_clipped_kernel (momentum_kernel's
// body with that scale; returns at once where the sum was not finite).  ws: grad_norm_ws_bytes(n) bytes, 16-byte aligned.
// The grid of the norm pass is a function of n alone, so the summation tree is too: bit-reproducible.
constexpr int GRAD_NORM_BLOCK = 256;              // threads of a block = 4-float groups of one block's pass
constexpr int GRAD_NORM_GRID_CAP = 256 * 16;      // blocks: the update's own cap
constexpr int GRAD_NORM_UNROLL = 4;                // passes of the grid whose loads a thread issues together: the main loop of the norm
                                                  // kernel runs while GRAD_NORM_UNROLL whole passes remain, a one-pass loop takes the rest
size_t grad_norm_ws_bytes(size_t n);
void momentum_update_clipped(float* w, float* acc, const float* g, size_t n, float lr, float momentum, float gscale, float max_norm,
                             void* ws, float* report, hipStream_t s);
// the first two of those launches alone (ProfScope "grad_norm"): what they leave at the head of ws, for the update that follows
struct ClipState {
    float gscale;       // grad_scale * factor
    unsigned skip;      // the sum of squares was not finite: the update touches nothing
    unsigned pad[2];
};
static_assert(sizeof(ClipState) == 16, "the partials behind it are read as aligned doubles");
void grad_norm_pass(const float* g, size_t n, float gscale, float max_norm, void* ws, float* report, hipStream_t s);

// ---- AdamW (optim.hip, compiled without fused multiply-add; contract in include/ssdvgg_hip.h "update rule").
// m: the momentum arena as first moment; v: the second moment; both n floats.  Decoupled decay on elements [0, n_decay), any
// n_decay in 0..n.  t >= 1: the count of AdamW updates since the state was zeroed, this one included.  The host scalars (1 - beta,
// the two bias corrections, lr * decay) are computed here in double and rounded to float once.  max_norm == 0: one launch,
// adamw_kernel<false> (ProfScope "adamw_update").  Otherwise grad_norm_pass and adamw_kernel<true> ("adamw_update_clipped"), which
// reads {scale, skip} from ws like momentum_clipped_kernel.  adamw_check refuses hyper-parameters outside their ranges
// (beta1, beta2, eps, decay in that order).
constexpr int UPDATE_MOMENTUM = 0, UPDATE_ADAMW = 1;      // SSD_UPDATE_* of the C ABI (api.hip asserts the match)
constexpr int ADAMW_BLOCK = 256;                 // one pass of the grid is ADAMW_BLOCK * ADAMW_GRID_CAP * 4 floats
constexpr int ADAMW_GRID_CAP = 256 * 16;
void adamw_check(float b1, float b2, float eps, float decay);
void adamw_update(float* w, float* m, float* v, const float* g, size_t n, size_t n_decay, float lr, float b1, float b2, float eps,
                  float decay, long long t, float gscale, float max_norm, void* ws, float* report, hipStream_t s);
// ---- weight EMA (optim.hip; contract in include/ssdvgg_hip.h "weight EMA").  e, w (a, b): n floats, n a multiple
// of 4.  t >= 0: the count of EMA updates before this one; the host computes omd = (float)(1 - min(decay, (1 + t) / (10 + t))) in
// double.  ema_update: one launch of ema_kernel (ProfScope "ema_update"), e -= omd * (e - w), adamw_update's launch shape.
// ema_swap: one launch of swap_kernel ("ema_swap"), the contents of a and b exchanged.  ema_check refuses a decay outside (0, 1).
void ema_check(float decay);
void ema_update(float* e, const float* w, size_t n, float decay, long long t, hipStream_t s);
void ema_swap(float* a, float* b, size_t n, hipStream_t s);

// gradients of a step without samples (a data-parallel rank whose shard of a short last batch is empty)
void null_gradients(const float* w, float* g, size_t nfilters, size_t n, float wd, hipStream_t s);
// fp32 gradient range <-> bf16 message buffer of the data-parallel all-reduce (halves the bytes that cross xGMI)
void grads_to_bf16(const float* g, void* out, size_t n, hipStream_t s);
void grads_from_bf16(const void* in, float* g, size_t n, hipStream_t s);

void clock_monitor(unsigned* out, int nsamples, unsigned period, hipStream_t s);
void fill_zero(void* p, size_t bytes, hipStream_t s);

}  // namespace ssd
