// Drawing detections on images in HBM (annotate.hip) -- host interface.
#pragma once
#include "common.h"
#include "../../include/ssdvgg_hip.h"

namespace ssd {
struct AnnotateStyle;      // class colours + names on one GPU (ssd_annotate_style_create)
AnnotateStyle* annotate_style_create(int device, int num_classes, const unsigned char* colors_bgr, const char* names32);
void annotate_style_destroy(AnnotateStyle* s);
int annotate_style_device(const AnnotateStyle* s);
size_t annotate_ws_bytes(int b, int out_cap);
void annotate_rect(const int box1000[4], int w, int h, int out[4]);
void annotate_glyph(int ch, unsigned char rows[7]);
void annotate_batch(const void* src_dev, bool src_f32, const ssd_annotate_image* images_host, int b, const int* count_dev,
                    const int* cls_dev, const int* box_dev, int out_cap, bool grid1000, const AnnotateStyle* style, bool rgb_out,
                    void* dst_dev, bool dst_f32, void* ws, hipStream_t s);
}  // namespace ssd
