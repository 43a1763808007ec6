// Average precision on the GPU (metrics.hip): the reference's protocol, VOC07 with difficult objects, VOC12 all-point AP,
// and the device-side accumulator that collects a run's detections behind each detection pass.
#pragma once
#include "common.h"

namespace ssd {

constexpr int AP_MAX_THRESHOLDS = 10;
enum { AP_REFERENCE = 0, AP_VOC07 = 1, AP_VOC12 = 2 };

// Device-visible inputs of one AP computation.  Ground truth rows are grouped by ascending sample id.
struct APInput {
    int n_det, n_gt, ncls;
    const float* det_box;      // [n_det][4] xmin,xmax,ymin,ymax (the reference casts them to float32)
    const float* det_conf;
    const int* det_cls;
    const int* det_sample;
    const double* gt_box;      // [n_gt][4]
    const int* gt_cls;
    const int* gt_sample;
    const unsigned char* gt_flags;      // [n_gt]: 1 = difficult
};

// Runs the count / sort / walk kernels on `s`, waits for it and copies ap [n_thr][ncls] and present [ncls] to the host.
void average_precision_run(const APInput& in, int protocol, int n_thr, const double* minoverlaps, double* ap_out, int* present_out,
                           hipStream_t s);

// COCO's box evaluation (metrics.hip, "COCO").  The arrays of APInput (gt_flags: bit 1 = crowd, nonzero = ignored) with the
// annotations' areas in pixels^2, W*H/1e6 of every image and the first ground-truth row of every sample.
constexpr int COCO_AREAS = 4, COCO_GROUPS = 6;      // all / small / medium / large at maxDet 100; then all at maxDet 1 and 10
struct COCOInput {
    APInput in;
    int n_samples;
    const double* gt_area;          // [n_gt]
    const double* sample_scale;     // [n_samples]
    const int* gt_first;            // [n_samples + 1]
};

// Runs count / sort / coco walk on `s`, waits and copies ap [4][n_thr][ncls], ar [6][n_thr][ncls], present [4][ncls] to the host.
// gt_sample_host: the host's copy of in.gt_sample (ascending), from which gt_first is made when c.gt_first is null.
void coco_eval_run(const COCOInput& c, const int* gt_sample_host, int n_thr, const double* thresholds, double* ap_out, double* ar_out,
                   int* present_out, hipStream_t s);

// Measurements: enable != 0 puts HIP events around the count, sort and walk stages of every later computation in this process;
// ms_out [3] (may be null) receives the stage times of the last timed one.
void ap_kernel_times(int enable, double* ms_out);

// A run's detections in HBM.  Everything it takes from HIP is owned by `hip` and freed with it.
class APAccumulator {
public:
    APAccumulator(int device, int num_classes);
    int device() const { return device_; }
    int num_classes() const { return ncls_; }
    void clear();
    void add_dev(int b, int out_cap, const int* count_dev, const float* conf_dev, const int* cls_dev, const int* box_dev, int n_gt,
                 const double* gt_box, const int* gt_cls, const int* gt_image, const unsigned char* gt_flags, hipStream_t s);
    void add_host(int n_det, const float* det_box, const float* det_conf, const int* det_cls, const int* det_sample, int n_samples,
                  int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample, const unsigned char* gt_flags);
    // the _coco appends: the same with the annotations' areas and the images' W*H/1e6; the flags keep the crowd bit
    void add_dev_coco(int b, int out_cap, const int* count_dev, const float* conf_dev, const int* cls_dev, const int* box_dev, int n_gt,
                      const double* gt_box, const int* gt_cls, const int* gt_image, const unsigned char* gt_flags, const double* gt_area,
                      const double* sample_scale, hipStream_t s);
    void add_host_coco(int n_det, const float* det_box, const float* det_conf, const int* det_cls, const int* det_sample, int n_samples,
                       int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample, const unsigned char* gt_flags,
                       const double* gt_area, const double* sample_scale);
    void compute_coco(int n_thr, const double* thresholds, double* ap_out, double* ar_out, int* present_out, long long* n_det,
                      long long* n_dropped);
    void counts(long long* n_det, long long* n_dropped);      // waits for the appends
    void fetch(long long cap, float* det_box, float* det_conf, int* det_cls, int* det_sample, long long* n_det);
    void compute(int protocol, int n_thr, const double* minoverlaps, double* ap_out, int* present_out, long long* n_det,
                 long long* n_dropped);
    long long samples() const { return samples_; }

private:
    struct Store { float* box = nullptr; float* conf = nullptr; int* cls = nullptr; int* sample = nullptr; };
    void reserve(long long extra, hipStream_t s);
    void sync();
    void release_retired();
    void push_gt(int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample, const unsigned char* gt_flags, int n_samples,
                 const char* what, const double* gt_area = nullptr, const double* sample_scale = nullptr);
    HipOwner hip_;
    int device_, ncls_;
    Store st_;
    long long cap_ = 0, bound_ = 0, samples_ = 0;      // bound_: the host's upper bound of the device-side end
    int* words_ = nullptr;                             // device: [0] end, [1] dropped detections
    std::vector<void*> retired_;                       // outgrown buffers, freed at the next wait
    hipStream_t last_ = nullptr;
    std::vector<double> gt_box_;
    std::vector<int> gt_cls_, gt_sample_;
    std::vector<unsigned char> gt_flags_;
    std::vector<double> gt_area_, sample_scale_;       // of the _coco appends
    long long plain_samples_ = 0;                      // samples appended without areas / scales: they bar compute_coco
};

}  // namespace ssd
