// Baseline JPEG encode (jpeg_enc.hip): colour conversion + downsampling + forward DCT + quantisation on the GPU, Huffman coding
// and file framing on the host -- host interface.
#pragma once
#include "common.h"
#include "../../include/ssdvgg_hip.h"

namespace ssd {
void jpeg_quant_tables(int quality, unsigned short* luma, unsigned short* chroma);
size_t jpeg_enc_coef_bytes(const int* shapes, int n, int sampling);
size_t jpeg_enc_ws_bytes(const int* shapes, int n, int sampling);
void jpeg_encode_batch(const unsigned char* src_dev, size_t src_bytes, const unsigned long long* src_offs, const int* shapes, int n,
                       int quality, int sampling, short* coef_dev, size_t coef_bytes, ssd_jpeg_desc* descs_out, void* ws,
                       size_t ws_bytes, hipStream_t s);
size_t jpeg_file_bound(const ssd_jpeg_desc& d);
// what the Huffman stage on the GPU (jpeg_huff.hip) shares with the host stage: the descriptor rules, the SSD_JPEG_HEADER_BYTES in
// front of the scan, and the Annex K codes as code | length << 16 ([0] luma, [1] chroma; DC by category, AC by run << 4 | size)
void jpeg_require_enc_desc(const ssd_jpeg_desc& d, size_t coef_bytes, int i);
void jpeg_file_header(const ssd_jpeg_desc& d, unsigned char* out);
void jpeg_huff_code_tables(unsigned dc[2][16], unsigned ac[2][256]);
size_t jpeg_entropy_encode(const short* coef, size_t coef_bytes, const ssd_jpeg_desc& d, unsigned char* out, size_t out_cap);
void jpeg_entropy_encode_batch(const short* coef, size_t coef_bytes, const ssd_jpeg_desc* descs, int n, int threads,
                               unsigned char* out, size_t out_bytes, const unsigned long long* out_offsets,
                               unsigned long long* out_sizes);
}  // namespace ssd
