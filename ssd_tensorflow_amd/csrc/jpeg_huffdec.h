// Baseline JPEG Huffman decoding on the GPU (jpeg_huffdec.hip): from the files' bytes in one device buffer to the
// int16 coefficients jpeg_idct_kernel reads -- host interface.
#pragma once
#include "common.h"
#include "../../include/ssdvgg_hip.h"

namespace ssd {
size_t jpeg_huffdec_ws_bytes(const ssd_jpeg_plan* plans, const ssd_jpeg_desc* descs, int n);
void jpeg_huffdec_batch(const unsigned char* files_dev, size_t files_bytes, const ssd_jpeg_plan* plans, const ssd_jpeg_desc* descs,
                        int n, short* coef_dev, size_t coef_bytes, ssd_jpeg_huffdec_rec* recs_dev, void* ws, size_t ws_bytes,
                        int max_rounds, hipStream_t s);
}  // namespace ssd
