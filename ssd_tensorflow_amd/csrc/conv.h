// im2col-free direct convolution on gfx950 fp32 MFMA -- host interface.
// Replaces the TensorFlow kernels behind tf.nn.conv2d / atrous_conv2d / bias_add /
// relu at ssdvgg.py:48-50, 61-62, 260-262, 287-290 and their gradients.
#pragma once
#include <vector>
#include "common.h"

namespace ssd {

// NHWC activations, HWIO filters ([KH*KW][Ci][Co] row-major).  Every channel
// count is a multiple of 4 except Ci == 3 (conv1_1, scalar-gather path).
struct ConvDesc {
    int B, Hi, Wi, Ci;
    int Ho, Wo, Co;
    int KH, KW, stride, dil;
    int pad_h, pad_w;   // zero rows/cols BEFORE the image (TF SAME: total/2; VALID: 0)
};

void conv_fwd(const ConvDesc& d, const float* x, const float* w, const float* bias,
              float* y, bool relu, hipStream_t s);

// dx = conv^T(dy, w).  mask != nullptr: dx is zeroed where mask <= 0 (relu of the
// producer, mask has dx's shape).  accumulate: dx += (before the mask).
void conv_dgrad(const ConvDesc& d, const float* dy, const float* w, float* dx,
                const float* mask, bool accumulate, hipStream_t s);

// dw = x^T * dy (+ weight_decay * w), dbias = column sums of dy.
// Two stages: split-M partial slabs into ws, then a fixed-order reduce (deterministic).
size_t conv_wgrad_ws_floats(const ConvDesc& d);
void conv_wgrad(const ConvDesc& d, const float* x, const float* dy, float* dw, float* dbias,
                const float* w, float weight_decay, float* ws, hipStream_t s);

// ---- 2x2 stride-2 max-pool fused into its neighbours (round 5; ops.h maxpool_*_rec is the unfused form) ----
// Forward: y_pool[b][oh/2][ow/2][c] = max over the window of relu(conv + bias), first maximum in scan order wins, cells outside
// the image never (TF SAME, no leading padding); rec (may be nullptr) = the pool's 12-bit record per (window, 4 channels).  The
// convolution's own output is NOT written.  3x3 / stride 1 / SAME convolutions.  Bit-identical to conv_fwd + maxpool_fwd_rec.
bool conv_fwd_pool_supported(const ConvDesc& d);
void conv_fwd_pool(const ConvDesc& d, const float* x, const float* w, const float* bias, float* y_pool, void* rec, hipStream_t s);
// Backward: the data gradient of a conv whose INPUT is the pooled tensor, scattered through the pool's record into the
// [B, UH, UW, Ci] gradient of the pool's input: cell = the recorded first maximum and (relu of the producer) the maximum was
// positive ? dx : 0; every cell of dx_unpooled is written.  Bit-identical to conv_dgrad + maxpool_bwd_rec(relu_mask = true).
bool conv_dgrad_unpool_supported(const ConvDesc& d);
void conv_dgrad_unpool(const ConvDesc& d, const float* dy, const float* w, float* dx_unpooled, const void* rec, int UH, int UW,
                       hipStream_t s);

// dedicated fp32 first-layer forward (conv_first.hip): Ci*taps <= 32, Co == 64
bool conv_first_fwd_f32_applicable(const ConvDesc& d);
void conv_first_fwd_f32(const ConvDesc& d, const float* x, const float* w, const float* bias, float* y, bool relu, hipStream_t s);
// dedicated fp32 first-layer weight gradient (conv_first.hip): Ci*taps <= 30, Co == 64; operands straight from global memory
bool conv_first_wgrad_f32_applicable(const ConvDesc& d);
size_t conv_first_wgrad_f32_ws_floats(const ConvDesc& d);
void conv_first_wgrad_f32(const ConvDesc& d, const float* x, const float* dy, float* dw, float* dbias, const float* w,
                          float weight_decay, float* ws, hipStream_t s);

// ---- Round 6: Winograd F(4x4, 3x3) for the fp32 3x3 / stride 1 / SAME layers (winograd.hip) ------------------------------------------
// Transformed tensors are position-major [36][tiles][C]; *_ps = elements between two positions (so a forward lane can own a row range
// of a full-batch tensor).  U = the filter's transform [36][Ci][Co] (forward), Uflip = [36][Co][Ci] of the rotated filter (data gradient).
bool wino_applicable(const ConvDesc& d);
int wino_tiles(const ConvDesc& d);                         // B * ceil(H / 4) * ceil(W / 4) (dilation d: per residue class, see winograd.hip)
int wino_kpad(int c);                                      // c rounded up to the GEMMs' k granularity (32): row length of the transformed dy,
                                                           // rows per position of Uflip (pad rows / columns are zero; Uflip's are the caller's to clear once)
void wino_filter(const ConvDesc& d, const float* w, float* U, float* Uflip, hipStream_t s);      // either may be nullptr
// every Winograd layer's filter transforms in one launch per kind (the step runs them at the start of forward, beside conv1_x)
struct WinoFilterPlan {
    static constexpr int MAX = 24;
    struct Item {
        const float* w;
        float *U, *Uf;
        int Ci, Co, Cop, blk0;
        int tblk0;      // the flipped transform's first workgroup: one per 32 ci x 32 co tile
    } it[MAX];
    int n = 0, blocks = 0, tblocks = 0;
    double elems = 0;
    void add(const float* w, float* U, float* Uf, int Ci, int Co);
};
// flip_lanes_ci: the flipped transform as the kernel with lanes along ci and no LDS staging (the same bits; also SSD_WINO_FILTER_LDS=0)
void wino_filter_plan(const WinoFilterPlan& plan, bool forward, bool flipped, hipStream_t s, bool flip_lanes_ci = false);
size_t wino_fwd_ws_floats(const ConvDesc& d);              // Mws: 36 * tiles * Co
// y = relu?(conv(x) + bias); V [36][.][Ci] receives the input's transform (kept by a training step for wino_wgrad).  y_pool != nullptr:
// the fused 2x2 pool of conv_fwd_pool instead of y (same values, same record).
// relu_bits (optional, tiles * Ci / 4 64-bit words): which of x's values are positive, per tile and 4 channels -- what wino_dgrad of the
// SAME layer takes as mask_bits in place of a second read of x
// ref_geom (here, wino_bwd_transform, wino_wgrad): the reference launch geometry of winograd.hip (raster-order input transform, the
// one-thread-per-(ci, 4 co) reduce) -- the same bits, kept for the bit-identity test and same-box A/Bs; SSD_WINO_GEOMETRY=0 forces it
void wino_fwd(const ConvDesc& d, const float* x, const float* U, const float* bias, float* y, bool relu, float* V, size_t v_ps,
              float* Mws, float* y_pool, void* pool_rec, hipStream_t s, void* relu_bits = nullptr, bool two_launch = false,
              bool ref_geom = false);
// dy -> Yt (B^T dy B, the data gradient's operand) and / or Ya (A dy A^T, the weight gradient's), each [36][tiles][wino_kpad(Co)]; nullptr skips one
// Both: one kernel that reads dy once (the same bits as the two single forms); two_launch or SSD_WINO_DUAL=0: the two single launches
void wino_bwd_transform(const ConvDesc& d, const float* dy, float* Yt, float* Ya, hipStream_t s, bool ref_geom = false, bool two_launch = false);
size_t wino_dgrad_ws_floats(const ConvDesc& d);            // Xws: 36 * tiles * Ci
// conv_dgrad's semantics (mask, accumulate) from the transformed dy; unpool_rec != nullptr: conv_dgrad_unpool's
void wino_dgrad(const ConvDesc& d, const float* Yt, const float* Uflip, float* dx, const float* mask, bool accumulate, float* Xws,
                const void* unpool_rec, int UH, int UW, hipStream_t s, const void* mask_bits = nullptr, bool two_launch = false);
size_t wino_wgrad_ws_floats(const ConvDesc& d);
// conv_wgrad's semantics from the forward's V and the transformed dy
void wino_wgrad(const ConvDesc& d, const float* V, size_t v_ps, const float* Ya, float* dw, float* dbias, const float* w,
                float weight_decay, float* ws, hipStream_t s, bool ref_geom = false);

// ---- convolutions with more than 9 taps (conv_bigk.hip): the fc graph's 7x7 fc6 -------------------------------------------------
// Stride 1, dilation 1, SAME; channel counts multiples of 4 (fp32) / 8 (bf16).  conv_fwd / conv_dgrad / conv_wgrad and their bf16 forms
// dispatch here when KH * KW > 9 (the gather kernels carry 9-entry tap tables); the weight gradient needs no workspace.
bool conv_bigk(const ConvDesc& d);
double conv_bigk_useful_flops(const ConvDesc& d);          // 2 * Ci * Co * the (pixel, tap) pairs that land inside the image
void conv_bigk_fwd(const ConvDesc& d, const float* x, const float* w, const float* bias, float* y, bool relu, hipStream_t s);
void conv_bigk_dgrad(const ConvDesc& d, const float* dy, const float* w, float* dx, const float* mask, bool accumulate, hipStream_t s);
void conv_bigk_wgrad(const ConvDesc& d, const float* x, const float* dy, float* dw, float* dbias, const float* w, float weight_decay,
                     hipStream_t s);

// ---- bf16 configuration (conv_bf16.hip): bf16 activations / gradients / filter mirrors, fp32 accumulate ----
struct bf16_t;

// conv1_1 (Ci = 3) stays on the fp32 kernels: fp32 image and master filter in, bf16 out / bf16 dy in
void conv_fwd_smallc_bf16out(const ConvDesc& d, const float* x, const float* w, const float* bias, bf16_t* y, bool relu,
                             hipStream_t s);
void conv_wgrad_smallc_bf16dy(const ConvDesc& d, const float* x, const bf16_t* dy, float* dw, float* dbias, const float* w,
                              float weight_decay, float* ws, hipStream_t s);

// dedicated first-layer kernels (conv_first_bf16.hip): Ci*taps <= 32 and Co == 64; image and filter are rounded to bf16
void conv_first_fwd_bf16(const ConvDesc& d, const float* x, const float* w, const float* bias, bf16_t* y, bool relu, hipStream_t s);
size_t conv_first_wgrad_bf16_ws_floats(const ConvDesc& d);
void conv_first_wgrad_bf16(const ConvDesc& d, const float* x, const bf16_t* dy, float* dw, float* dbias, const float* w,
                           float weight_decay, float* ws, hipStream_t s);

// the bf16 forms of conv_bigk_* (fp32 accumulation; the filter operands are the bf16 mirrors below)
void conv_bigk_fwd_bf16(const ConvDesc& d, const bf16_t* x, const bf16_t* w_oi, const float* bias, void* y, bool y_f32, bool relu,
                        hipStream_t s);
void conv_bigk_dgrad_bf16(const ConvDesc& d, const bf16_t* dy, const bf16_t* w_io, bf16_t* dx, const bf16_t* mask, bool accumulate,
                          hipStream_t s);
void conv_bigk_wgrad_bf16(const ConvDesc& d, const bf16_t* x, const bf16_t* dy, float* dw, float* dbias, const float* w,
                          float weight_decay, hipStream_t s);

// One launch mirrors every layer's fp32 filter [tap][Ci][Co] as bf16 in the same order (io, the data
// gradient's operand) and transposed [tap][Co][Ci] (oi, the forward operand), at the same offsets.
struct FilterCastPlan {
    static constexpr int MAX_LAYERS = 48;
    struct Layer {
        size_t off;
        int taps, ci, co;
    } L[MAX_LAYERS];
    int n = 0;
    void add(size_t off, int taps, int ci, int co);
};
void cast_filters(const FilterCastPlan& plan, const float* w, bf16_t* io, bf16_t* oi, hipStream_t s);

// launches of the same shape the caller runs side by side on other streams (tile choice: conv_bf16.hip gather_rows_n64)
extern thread_local int g_conv_lanes;
// y: bf16 [B,Ho,Wo,Co], or fp32 when y_f32 (the multibox heads feed the fp32 loss)
void conv_fwd_bf16(const ConvDesc& d, const bf16_t* x, const bf16_t* w_oi, const float* bias, void* y, bool y_f32, bool relu,
                   hipStream_t s);
void conv_dgrad_bf16(const ConvDesc& d, const bf16_t* dy, const bf16_t* w_io, bf16_t* dx, const bf16_t* mask, bool accumulate,
                     hipStream_t s);
// the bf16 forms of the fused pool (above); forward: est. fraction of the tile rows that carry pixels is part of "supported"
bool conv_fwd_pool_bf16_supported(const ConvDesc& d);
void conv_fwd_pool_bf16(const ConvDesc& d, const bf16_t* x, const bf16_t* w_oi, const float* bias, bf16_t* y_pool, void* rec, hipStream_t s);
bool conv_dgrad_unpool_bf16_supported(const ConvDesc& d);
void conv_dgrad_unpool_bf16(const ConvDesc& d, const bf16_t* dy, const bf16_t* w_io, bf16_t* dx_unpooled, const void* rec, int UH, int UW,
                            hipStream_t s);
// Round 5: the data gradient of the 64 -> 64 layer d (conv1_2) with the WEIGHT gradient of the first layer d1 below it (conv1_1:
// 3 input channels, 3x3) computed from the dx tiles while they are in LDS: dx is never written, conv1_1's own weight-gradient
// kernel is not launched.  dw1 / dbias1 = sum over pixels (+ weight_decay * w1), reduced from one slab per workgroup in ws
// (conv_dgrad_first_wgrad_bf16_ws_floats).  mask = the first layer's output (relu mask of dx).
bool conv_dgrad_first_wgrad_bf16_applicable(const ConvDesc& d, const ConvDesc& d1);
size_t conv_dgrad_first_wgrad_bf16_ws_floats(const ConvDesc& d1);
void conv_dgrad_first_wgrad_bf16(const ConvDesc& d, const bf16_t* dy, const bf16_t* w_io, const bf16_t* mask, const ConvDesc& d1,
                                 const float* image, float* dw1, float* dbias1, const float* w1, float weight_decay, float* ws,
                                 hipStream_t s);
size_t conv_wgrad_bf16_ws_floats(const ConvDesc& d);
void conv_wgrad_bf16(const ConvDesc& d, const bf16_t* x, const bf16_t* dy, float* dw, float* dbias, const float* w,
                     float weight_decay, float* ws, hipStream_t s);

// ---- Round 6: the latency-bound tail (conv9_1 ... conv11_2 / conv12_2 and the small maps' heads) as one launch per direction ----
// tail_bf16.hip: a chain of convolution stages (forward, or data gradients in backward order), each image's chain walked by ONE
// workgroup with workgroup barriers between the stages -- nothing below the 10x10 map couples two images.  Pointers are those of
// the FIRST image of the launch; d.B is ignored (nimg images, [nimg][H][W][C] tensors).
struct TailStage {
    ConvDesc d;             // the convolution's geometry (forward sense), as conv_fwd_bf16 / conv_dgrad_bf16 take it
    bool dgrad;             // false: dst = relu?(conv(src) + bias);  true: dst (+)= conv^T(src), masked by `mask` > 0
    const void* src;        // forward: x [.][Hi][Wi][Ci];  data gradient: dy [.][Ho][Wo][Co]   (bf16)
    const void* wgt_packed; // the stage's filter in the chain kernel's fragment order: tail_chain_pack_filter of the [tap][Co][Ci] mirror
                            // (forward) or of the [tap][Ci][Co] mirror (data gradient); tail_chain_packed_elems bf16 elements
    const float* bias;      // forward
    const void* mask;       // data gradient: the relu mask tensor (dx's shape, bf16) or nullptr
    void* dst;              // forward: y (bf16, or fp32 when out_f32);  data gradient: dx (bf16)
    bool relu, accum, out_f32;
};
int tail_chain_max_stages();
bool tail_chain_stage_supported(const ConvDesc& d);
size_t tail_chain_packed_elems(const ConvDesc& d, bool dgrad);
struct TailPackItem {
    ConvDesc d;
    bool dgrad;             // false: `mirror` is the [tap][Co][Ci] image (forward stage); true: the [tap][Ci][Co] image (data-gradient stage)
    const void* mirror;
    void* packed;
};
void tail_chain_pack_filters(const TailPackItem* items, int n, hipStream_t s);      // one launch
// The stage tables tail_chain_bf16 has uploaded into `owner`'s device memory, found again by content.  The caller keeps the store
// as long as the launches may run: a handle for its life (one table per direction and lane start), an op for the call.
struct TailTables {
    HipOwner& owner;
    std::vector<std::pair<std::vector<char>, const void*>> uploaded;
};
void tail_chain_bf16(const TailStage* stages, int nstages, int nimg, const char* label, hipStream_t s, TailTables& tables);
// The plan tail_chain_bf16 launches, as the host computes it (no HIP call; the stages' pointers are only keys: which stage's output
// is which stage's input).  All offsets and sizes are bytes of the workgroup's LDS: [0, TAIL_ZERO_BYTES) is the zero row, a feature
// map's region holds its pixel rows at a pitch of channels * 2 + 16 plus 256 bytes.  Throws what tail_chain_bf16 would.
constexpr int TAIL_ZERO_BYTES = 2560;        // the zero row: covers the widest pixel row (1024 channels) plus a group's immediates
constexpr int TAIL_LDS_MAX = 160 * 1024;
constexpr int TAIL_PLAN_MAX_TASKS = 64;
enum { TF_RELU = 1, TF_ACCUM = 2, TF_OUT_F32 = 4, TF_LOAD_IN = 8, TF_LOAD_OUT = 16, TF_KTAIL = 32 };
struct TailPlanStage {
    int flags;                              // TF_*
    int ntask, tiles, ksplit, ngroups, GPT; // ntask = tiles * ksplit; ngroups = taps * GPT groups of 4 k steps of 32 channels
    int in_off, in_bytes;                   // the gathered tensor's region
    int out_off, out_bytes;                 // the output's region (-1, 0: not kept in LDS)
    int scratch_off, scratch_bytes;         // the k-split partial sums
    unsigned tasks[TAIL_PLAN_MAX_TASKS][2]; // [0] = nb | mg << 8 | ks << 16 | nmb << 24,  [1] = g0 | g1 << 16
};
void tail_chain_plan(const TailStage* stages, int nstages, TailPlanStage* out, int* lds_total);
// the weight gradients of several small layers in ONE launch, each with a single pixel split and the direct epilogue
// (dw = x^T dy + weight_decay * w, dbias = column sums of dy): no slabs, no reduce launches
struct WgradGroupItem {
    ConvDesc d;
    const bf16_t* x;
    const bf16_t* dy;
    float* dw;
    float* dbias;
    const float* w;
};
int conv_wgrad_group_bf16_max();
void conv_wgrad_group_bf16(const WgradGroupItem* items, int n, float weight_decay, hipStream_t s);

// ---- fp8 inference kernels (conv_fp8.hip): OCP e4m3fn codes, one fp32 scale per activation tensor and per output channel ----
// (The four e4m3 convolutions below -- fp8 and mxfp8, up to 9 taps and 10 ... 121 -- are one kernel, one shape check and one host path:
// conv_fp8_detail.h.  The entry points differ in the format, the tap range they accept and the workgroup order.  The same header
// holds what the mxfp6 convolution shares with them -- the shape check (conv_quant_refusal), the host prologue, the launcher -- and the table of the two filter quantisers; mx_block.h holds the two MX code formats as traits and, once
// over them, the scale rule, the stand-alone quantiser, max-pooling and the pools' geometry check.  DESIGN.md 33.)
// code = RNE(clamp(v / s, -448, 448)); y = relu?(acc * (s_in * s_w[co]) + bias[co]) in fp32, then one of the output forms.
enum { FP8_OUT_BF16 = 0, FP8_OUT_F32 = 1, FP8_OUT_E4M3 = 2, FP8_OUT_BF16_E4M3 = 3 };
// KH * KW <= 9, Ci a multiple of 64, Co a multiple of 8, any stride / dilation / leading padding, no empty tensor, every tensor and the
// filter image below the 32-bit offsets; why (optional) = the reason text, a string literal
bool conv_fwd_fp8_supported(const ConvDesc& d, const char** why);
// the shapes on which the step executor prefers this kernel to conv_fwd_bf16 (Ci >= 256; measured: conv_fp8.hip)
bool conv_fwd_fp8_worthwhile(const ConvDesc& d);
// x8 [B,Hi,Wi,Ci] and w8 [tap][Co][Ci] e4m3; y: bf16 or fp32 [B,Ho,Wo,Co] (unused by FP8_OUT_E4M3), y8: e4m3 at scale s_out
// (FP8_OUT_E4M3 and FP8_OUT_BF16_E4M3).  Anything unsupported throws before a launch.
void conv_fwd_fp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* w8, float s_in, const float* s_w, const float* bias,
                  void* y, unsigned char* y8, int out_mode, float s_out, bool relu, hipStream_t s);
// The same contract for 10 ... 121 taps (KH, KW <= 11): the fc graph's 7x7 fc6.  9 taps or fewer are refused (conv_fwd_fp8 runs them).
bool conv_bigk_fwd_fp8_supported(const ConvDesc& d, const char** why);
// whether the step executor puts such a layer on e4m3 (SSD_FP8_BIGK, read per handle; the default is measured: conv_fp8.hip)
bool conv_bigk_fwd_fp8_worthwhile(const ConvDesc& d);
void conv_bigk_fwd_fp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* w8, float s_in, const float* s_w, const float* bias,
                       void* y, unsigned char* y8, int out_mode, float s_out, bool relu, hipStream_t s);
// One launch quantises every listed layer's fp32 filter [tap][Ci][Co] (element offset off in w) into its e4m3 image
// [tap][Co][Ci] (byte offset off8 in w8) with s_w[offs + co] = absmax_co / 448 (1 for an all-zero channel).
struct FilterQuantPlan {
    static constexpr int MAX_LAYERS = 48;
    struct Layer {
        size_t off, off8, offs;
        int taps, ci, co;
    } L[MAX_LAYERS];
    int n = 0;
    void add(size_t off, size_t off8, size_t offs, int taps, int ci, int co);
};
void quantize_filters_fp8(const FilterQuantPlan& plan, const float* w, unsigned char* w8, float* s_w, hipStream_t s);
// n values, bf16 or fp32 -> e4m3 at one scale
void quantize_fp8(const void* x, bool x_f32, size_t n, float scale, unsigned char* y8, hipStream_t s);
// *out = max(|x|) over the finite values (accumulate: the maximum with what *out holds); the reduction of calibration
void absmax_bf16(const bf16_t* x, size_t n, float* out, bool accumulate, hipStream_t s);
struct PoolDesc;
// max-pooling on e4m3 codes of either sign; C a multiple of 16; cells outside the image never win
void maxpool_fwd_fp8(const PoolDesc& d, const unsigned char* x8, unsigned char* y8, hipStream_t s);

// ---- mxfp8 inference kernels (conv_mxfp8.hip): e4m3 codes [B,H,W,C] + one E8M0 scale byte per pixel and 32 channels [B,H,W,C/32] ----
// scale rule on the bits of the block's fp32 absmax: x = clamp(E - 8 + (mantissa > 0x600000), -127, 127), byte x + 127 (an all-zero
// block: byte 0); codes = RNE(clamp(ldexp(v, -x), -448, 448)).  Filters as for fp8.  y = relu?(acc * s_w[co] + bias[co]) in fp32.
enum { FP8_OUT_MX = 4, FP8_OUT_BF16_MX = 5 };      // beside FP8_OUT_BF16 and FP8_OUT_F32: codes + scales / bf16 and codes + scales
// conv_fwd_fp8's eligibility (conv_fwd_fp8_supported); an MX output needs Co % 32 == 0.  xs is read in whole dwords: its allocation
// must be readable up to its size rounded up to 4 bytes.  Anything unsupported throws before a launch.
void conv_fwd_mxfp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* xs, const unsigned char* w8, const float* s_w,
                    const float* bias, void* y, unsigned char* y8, unsigned char* ys, int out_mode, bool relu, hipStream_t s);
// The same contract for 10 ... 121 taps (KH, KW <= 11): the fc graph's 7x7 fc6.  conv_bigk_fwd_fp8_supported's shapes,
// Co % 32 == 0 for an MX output mode, the scale tensors below the 32-bit offsets; 9 taps or fewer are refused (conv_fwd_mxfp8 runs them).
bool conv_bigk_fwd_mxfp8_supported(const ConvDesc& d, int out_mode, const char** why);
// whether the step executor puts such a layer on MX operands (SSD_MXFP8_BIGK, read per handle; unset = 0: conv_mxfp8.hip)
bool conv_bigk_fwd_mxfp8_worthwhile(const ConvDesc& d);
void conv_bigk_fwd_mxfp8(const ConvDesc& d, const unsigned char* x8, const unsigned char* xs, const unsigned char* w8, const float* s_w,
                         const float* bias, void* y, unsigned char* y8, unsigned char* ys, int out_mode, bool relu, hipStream_t s);
// bf16 or fp32 [rows][C] -> codes [rows][C] + scales [rows][C / 32]; C a multiple of 32 (mx_block.h: quantize_mx<MxE4M3>)
void quantize_mxfp8(const void* x, bool x_f32, size_t rows, int C, unsigned char* y8, unsigned char* ys, hipStream_t s);
// max-pooling of MX tensors: the maximum of the dequantised cells per channel, quantised again per block; C a multiple of 32
// (mx_block.h: maxpool_fwd_mx<MxE4M3>)
void maxpool_fwd_mxfp8(const PoolDesc& d, const unsigned char* x8, const unsigned char* xs, unsigned char* y8, unsigned char* ys, hipStream_t s);

// ---- mxfp6 inference kernels (conv_mxfp6.hip; the format: mx_block.h's MxE2M3): OCP MX FP6 E2M3 codes, 32 consecutive channels = one 24-byte string (code j
// in bits 6 j ... 6 j + 5, little-endian) + one E8M0 scale byte: activations [B,H,W,C/32][24] + [B,H,W,C/32], filters with blocks along
// Ci, w6 [tap][Co][Ci/32][24] + ws [tap][Co][Ci/32] and no per-channel scale ----
// scale rule on the bits of the block's fp32 absmax: x = clamp(E - 2 + (mantissa > 0x700000), -127, 127), byte x + 127 (an all-zero
// block: byte 0); codes = RNE(clamp(ldexp(v, -x), -7.5, 7.5)).  y = relu?(acc + bias[co]) in fp32.  Output modes: FP8_OUT_BF16, _F32,
// _MX, _BF16_MX, "MX" meaning this format.
// KH * KW <= 9, Ci a multiple of 64, Co a multiple of 8, any stride / dilation / leading padding, no empty tensor, every tensor and the
// filter below the 32-bit offsets; why (optional) = the reason text, a string literal.  There is no kernel for more than 9 taps.
bool conv_fwd_mxfp6_supported(const ConvDesc& d, const char** why);
// An MX output needs Co % 32 == 0.  xs and ws are read in whole dwords: their allocations must be readable up to their sizes rounded
// up to 4 bytes, and start at even addresses; the code buffers at multiples of 8.  Anything unsupported throws before a launch.
void conv_fwd_mxfp6(const ConvDesc& d, const unsigned char* x6, const unsigned char* xs, const unsigned char* w6, const unsigned char* ws,
                    const float* bias, void* y, unsigned char* y6, unsigned char* ys, int out_mode, bool relu, hipStream_t s);
// bf16 or fp32 [rows][C] -> codes [rows][C / 32][24] + scales [rows][C / 32]; C a multiple of 32 (mx_block.h: quantize_mx<MxE2M3>)
void quantize_mxfp6(const void* x, bool x_f32, size_t rows, int C, unsigned char* y6, unsigned char* ys, hipStream_t s);
// One launch quantises every listed layer's fp32 filter [tap][Ci][Co] (element offset off in w) into its code image (byte offset off8 in
// w6, a multiple of 8) and its scales (byte offset offs in ws); Ci a multiple of 32
void quantize_filters_mxfp6(const FilterQuantPlan& plan, const float* w, unsigned char* w6, unsigned char* ws, hipStream_t s);
// max-pooling of mxfp6 tensors: the maximum of the dequantised cells per channel, quantised again per block; C a multiple of 32
// (mx_block.h: maxpool_fwd_mx<MxE2M3>)
void maxpool_fwd_mxfp6(const PoolDesc& d, const unsigned char* x6, const unsigned char* xs, unsigned char* y6, unsigned char* ys, hipStream_t s);

}  // namespace ssd
