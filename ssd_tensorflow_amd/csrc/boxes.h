// Box math of the SSD hot path on gfx950: anchors, label encoding, decode, per-class NMS.
// Replaces the numpy loops of ssdutils.py:76-318 and transforms.py:57-114.
#pragma once
#include "common.h"

namespace ssd {

constexpr int PRESET_MAX_MAPS = 8;
constexpr int PRESET_MAX_TYPES = 8;

struct Preset {
    const char* name;
    int image_w, image_h;
    int nmaps;
    int map_size[PRESET_MAX_MAPS];
    double scale[PRESET_MAX_MAPS];
    int nratios[PRESET_MAX_MAPS];
    double ratios[PRESET_MAX_MAPS][4];
    double extra_scale;
    int num_anchors;
    // derived
    int ntypes[PRESET_MAX_MAPS];                          // 2 + nratios
    int off[PRESET_MAX_MAPS + 1];                         // first anchor of each map
    double bw[PRESET_MAX_MAPS][PRESET_MAX_TYPES];         // box sizes (host libm sqrt: correctly rounded)
    double bh[PRESET_MAX_MAPS][PRESET_MAX_TYPES];
};

// ssdutils.py:70-73; throws ssd::Error("No such preset: ...") like the reference's RuntimeError.
const Preset& get_preset(const char* name);

// [A][4] f64 (cx, cy, w, h) and [A][4] i32 (xmin, xmax, ymin, ymax on the 1000 grid), device.
void anchors_device(const Preset& p, double* anchors, int* anchors_abs, hipStream_t s);

// jaccard_overlap of one box vs n boxes (f64, +1 pixel convention); device pointers
void jaccard_device(const double* box, const double* arr, int n, double* iou, hipStream_t s);

// LabelCreatorTransform for a batch.  gt [ntot][4] f64 (cx,cy,w,h), cls [ntot], offsets [B+1]
// (CSR) all device; anchors/anchors_abs from anchors_device.  vec [B][A][C+5] f32 device.
size_t encode_labels_ws_bytes(int ntot);
void encode_labels(const Preset& p, int num_classes, const double* anchors, const int* anchors_abs, const double* gt,
                   const int* cls, const int* offsets, int B, int ntot, float* vec, void* ws, hipStream_t s);
// The same with a matching rule.  MATCH_REFERENCE: the encoder above, kernel for kernel.  MATCH_PAPER: first
// every box is matched one-to-one to the free anchor it overlaps best, whatever the IoU (greedy by IoU; ties: lower
// anchor, then lower box), then the remaining anchors take their best box above 0.5.  match_out [B][A] (device, may be
// null): the winning box's index within its image, -1 for a background row; filled under both rules.
// ws: encode_labels_ws_bytes_ex(ntot, B, match) bytes.  Any other `match` fails (require_match) before anything is enqueued.
constexpr int MATCH_REFERENCE = 0, MATCH_PAPER = 1;
void require_match(int match);
size_t encode_labels_ws_bytes_ex(int ntot, int B, int match);
void encode_labels_ex(const Preset& p, int num_classes, const double* anchors, const int* anchors_abs, const double* gt,
                      const int* cls, const int* offsets, int B, int ntot, float* vec, int* match_out, int match, void* ws,
                      hipStream_t s);

// decode_boxes + suppress_overlaps (+ the caller's [:max_out]) for a batch.
struct DetectOut {
    int* count;    // [B] boxes kept (before the out_cap clip)
    float* conf;   // [B][out_cap]
    int* cls;      // [B][out_cap]
    int* idx;      // [B][out_cap] anchor index
    int* box;      // [B][out_cap][4] xmin,xmax,ymin,ymax: normalize_box's integers
};
size_t detect_ws_bytes(int B, int A);
// nms = false: decode_boxes only (confidence order, nothing suppressed)
void detect(int A, int num_classes, const double* anchors, const float* pred, int B, float conf_thr, int cap,
            int max_out, int out_cap, bool nms, const DetectOut& out, void* ws, hipStream_t s);

// DetectionOutput: every (anchor, foreground class) pair with !(conf < conf_thr) is a candidate; per class the
// best nms_top_k (confidence descending, ties by lower anchor), greedy NMS per class at the reference's 0.45, then the best
// keep_top_k of the image by (confidence descending, anchor ascending, class ascending), written in THAT order (global
// confidence order, not detect()'s class groups).  out.count may exceed out_cap; rows past out_cap are clipped.
// nms_top_k, keep_top_k in 1..1024; conf_thr finite and >= 0.  Negative zero and NaN in the class columns are outside the
// contract (inputs are softmax outputs).  pred is not modified.  Asynchronous on s, no host wait, deterministic; every limit
// (and ws_bytes) is checked before anything is enqueued.
//   ws bytes = align256(4 b C) + align256(8 b C nms_top_k) + 16 b C nms_top_k
// `nms` replaces the greedy suppression by Soft-NMS: ssd_nms_params of the public header, whose comment is the
// contract.  kind = NMS_HARD (the default argument) launches the kernels of the hard rule and reads no other field.
struct NmsParams { int kind; float iou_thr, sigma, min_score; };
constexpr int NMS_HARD = 0, NMS_SOFT_LINEAR = 1, NMS_SOFT_GAUSSIAN = 2;
void nms_params_check(const char* who, const NmsParams* nms);      // kind, iou_thr (linear), sigma (gaussian), min_score: in this order
size_t detection_output_ws_bytes(int B, int num_classes, int nms_top_k);
void detection_output_check(int A, int num_classes, int B, float conf_thr, int nms_top_k, int keep_top_k, int out_cap);      // the limits alone
void detection_output(int A, int num_classes, const double* anchors, const float* pred, int B, float conf_thr, int nms_top_k,
                      int keep_top_k, int out_cap, const DetectOut& out, void* ws, size_t ws_bytes, hipStream_t s,
                      const NmsParams& nms = NmsParams{NMS_HARD, 0.f, 0.f, 0.f});
// Soft-NMS alone on one list of n <= 1024 boxes [n][4] i32 on the 1000 grid (device pointers): the picks' input indices and
// decayed scores in pick order, *n_keep their number.
void soft_nms_boxes_device(int n, const int* boxes, const float* conf, const NmsParams& nms, int* order_out, float* conf_out, int* n_keep,
                           hipStream_t s);

// non_maximum_suppression / suppress_overlaps on an arbitrary list: boxes [n][4] i32 (xmin,xmax,ymin,ymax),
// conf [n], group [n] (0..ngroups-1); keep [n+1]: keep[0] = count, then the selected input indices in output order.
size_t nms_boxes_ws_bytes(int n, int ngroups);
void nms_boxes_device(int n, int ngroups, const int* boxes, const float* conf, const int* group, double thr, int* keep, void* ws,
                      hipStream_t s);

// Tiled detection: the decode_boxes records of a picture's tiles -> one detection list per picture.
// MergeTile is ssd_tile of the public header: a window (x0, y0, w, h) of a picture of img_w x img_h source pixels,
// interior = which of its edges lie inside the picture (1 left, 2 right, 4 top, 8 bottom), image = the picture's index.
struct MergeTile { int x0, y0, w, h, img_w, img_h, interior, image; };
constexpr int MERGE_MAX_TILES = 256;       // tiles of one picture (8 bits of the sort key)
constexpr int MERGE_MAX_CAND = 32768;      // tiles of one picture * tile_cap (one survivor flag each in LDS)
constexpr int MERGE_LDS_KEYS = 2048;       // up to this many candidates (rounded up to a power of two) the sort runs in LDS
constexpr int MERGE_MAX_SIDE = 1000000;    // picture side: keeps 1000 * origin + 999 * extent below 2^31
size_t merge_tiles_ws_bytes(int n_tiles, int tile_cap);
// tiles: HOST array, pictures ascending 0 .. n_images-1 (copied by the call); count [n_tiles], conf / cls / idx [n_tiles][tile_cap],
// box [n_tiles][tile_cap][4] as detect() writes them with nms = false and out_cap = tile_cap; the outputs as DetectOut per
// picture plus tile_out (index of the tile inside its picture); conf_out, idx_out, tile_out may be null.  box and box_out
// 16-byte aligned.  Asynchronous on s; every limit is checked before anything is enqueued.
void merge_tiles_check(const MergeTile* tiles, int n_tiles, int n_images, int tile_cap, int out_cap);      // the limits alone
void merge_tiles(const MergeTile* tiles, int n_tiles, int n_images, int tile_cap, const int* count, const float* conf, const int* cls,
                 const int* idx, const int* box, int edge_margin, int max_out, int out_cap, int* count_out, float* conf_out,
                 int* cls_out, int* idx_out, int* tile_out, int* box_out, void* ws, hipStream_t s);

// Tiled DetectionOutput: every tile decoded as detection_output decodes an image (per class the best nms_top_k
// candidates, NO suppression inside a tile), edge drop, the picture's grid, then per class the best nms_top_k of the PICTURE
// through one greedy NMS, and the best keep_top_k of the picture across classes, in the order of the unique key
//   conf bits << 32 | (255 - tile) << 24 | (32767 - anchor) << 8 | (127 - class)      (descending).
// detout_tiles_add decodes the b network inputs pred [b][A][C+5] = tiles first .. first + b - 1 of the table into the
// workspace (once per network batch); detout_tiles_merge turns the workspace into the merged-detection layout of merge_tiles
// (conf_out, idx_out, tile_out may be null).  tiles: HOST array of ALL n_tiles, as for merge_tiles.  Asynchronous on s, no
// atomics on memory; every limit is checked before anything is enqueued, and `who` (the entry point) starts every message.
//   ws bytes = align256(4 (8 n_tiles + n_images + 1)) + sum over L in {n_tiles C, n_images C} of
//              align256(4 L) + align256(8 L nms_top_k) + align256(16 L nms_top_k)
size_t detout_tiles_ws_bytes(int A, int num_classes, int n_tiles, int n_images, int nms_top_k);
void detout_tiles_add_check(const char* who, int A, int num_classes, const MergeTile* tiles, int n_tiles, int first, int b, float conf_thr,
                            int nms_top_k, std::vector<int>& head);                                           // the limits alone
void detout_tiles_merge_check(const char* who, int num_classes, const MergeTile* tiles, int n_tiles, int n_images, int nms_top_k,
                              int keep_top_k, int out_cap, std::vector<int>& head);                          // the limits alone
void detout_tiles_add(const char* who, int A, int num_classes, const double* anchors, const float* pred, const MergeTile* tiles,
                      int n_tiles, int first, int b, float conf_thr, int nms_top_k, int edge_margin, void* ws, size_t ws_bytes,
                      hipStream_t s);
void detout_tiles_merge(const char* who, int num_classes, const MergeTile* tiles, int n_tiles, int n_images, int nms_top_k, int keep_top_k,
                        int out_cap, int* count_out, float* conf_out, int* cls_out, int* idx_out, int* tile_out, int* box_out, void* ws,
                        size_t ws_bytes, hipStream_t s, const NmsParams& nms = NmsParams{NMS_HARD, 0.f, 0.f, 0.f});

}  // namespace ssd
