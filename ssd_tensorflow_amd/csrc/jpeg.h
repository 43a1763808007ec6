// Baseline JPEG decode (jpeg.hip): entropy stage on the host, dequantise + IDCT + upsample + colour on the GPU -- host interface.
#pragma once
#include "common.h"
#include "../../include/ssdvgg_hip.h"

namespace ssd {
// Header only.  Returns SSD_JPEG_OK / SSD_JPEG_UNSUPPORTED; corrupt input throws.  `desc` gets the geometry and the
// quantisation tables (coef_off relative to the file's own first coefficient, dst_off 0, max_l1 0).
int jpeg_parse_header(const unsigned char* bytes, size_t n, ssd_jpeg_desc* desc);
size_t jpeg_coef_bytes(const ssd_jpeg_desc& d);
// One file: header + Huffman stream into coef_out (cap_bytes of room).  Same return convention; an image with a block whose
// dequantised L1 norm exceeds SSD_JPEG_MAX_L1 is SSD_JPEG_UNSUPPORTED.
int jpeg_entropy_decode(const unsigned char* bytes, size_t n, short* coef_out, size_t cap_bytes, ssd_jpeg_desc* desc);
void jpeg_entropy_decode_batch(const unsigned char* const* files, const size_t* sizes, int n, int threads, short* coef_out,
                               const unsigned long long* offsets, ssd_jpeg_desc* descs, int* status_out);
// The scan plan of the device Huffman stage (jpeg_huffdec.hip): markers as jpeg_parse_header judges them, then the segments' byte
// ranges and the selected tables without decoding a bit.  SSD_JPEG_TO_HOST: no usable plan, jpeg_entropy_decode decides.
size_t jpeg_scan_segments(const unsigned char* bytes, size_t n);
int jpeg_scan_plan(const unsigned char* bytes, size_t n, ssd_jpeg_desc* desc, ssd_jpeg_plan* plan);
size_t jpeg_ws_bytes(const ssd_jpeg_desc* descs, int n);
void jpeg_decode_batch(const short* coef_dev, size_t coef_bytes, const ssd_jpeg_desc* descs, int n, unsigned char* dst_dev,
                       size_t dst_bytes, void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace ssd
