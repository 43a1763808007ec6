// GPU training augmentation (augment.hip) -- host interface.
#pragma once
#include "common.h"
#include "../../include/ssdvgg_hip.h"

namespace ssd {
size_t augment_ws_bytes(int b, int out_w, int out_h);
void augment_batch(const unsigned char* images_dev, const ssd_augment_params* params_host, int b, int out_w, int out_h, float* out_dev,
                   void* ws, hipStream_t s);
// several pictures per output sample: picture i lands in the rectangle cells_host[i] of its sample (ssd_augment_cells_dev)
size_t augment_cells_ws_bytes(int n_cells, int out_w, int out_h);
void augment_cells(const unsigned char* images_dev, const ssd_augment_params* params_host, const ssd_augment_cell* cells_host, int n_cells, int b,
                   int out_w, int out_h, float* out_dev, void* ws, hipStream_t s);
}  // namespace ssd
