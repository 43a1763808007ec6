// Baseline JPEG Huffman coding and file framing on the GPU (jpeg_huff.hip): from the int16 coefficients
// jpeg_fdct_kernel leaves to complete JFIF files in one device buffer -- host interface.
#pragma once
#include "common.h"
#include "../../include/ssdvgg_hip.h"

namespace ssd {
size_t jpeg_huff_ws_bytes(const ssd_jpeg_desc* descs, int n);
size_t jpeg_huff_out_bytes(const ssd_jpeg_desc* descs, int n);
void jpeg_huffman_batch(const short* coef_dev, size_t coef_bytes, const ssd_jpeg_desc* descs, int n, unsigned char* out_dev,
                        size_t out_bytes, ssd_jpeg_file_rec* files_dev, void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace ssd
