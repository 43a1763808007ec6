// extern "C" boundary of libssdvgg_hip.so (include/ssdvgg_hip.h).
#include "../../include/ssdvgg_hip.h"
#include "net.h"
#include "augment.h"
#include "annotate.h"
#include "jpeg.h"
#include "jpeg_enc.h"
#include "jpeg_huff.h"
#include "jpeg_huffdec.h"
#include "metrics.h"
#include <vector>
#include <map>
#include <memory>
#include <mutex>
#include <algorithm>

namespace ssd {
static thread_local std::string g_err;
void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}
const char* get_error() { return g_err.c_str(); }

thread_local Profiler* g_prof = nullptr;
thread_local hipEvent_t g_stop_event = nullptr;
hipEvent_t Profiler::get() {
    if (used == pool.size()) {
        hipEvent_t e;
        HIP_OK(hipEventCreate(&e));
        pool.push_back(e);
    }
    return pool[used++];
}
Profiler::~Profiler() {
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
}
ProfScope::ProfScope(const char* kernel, double flops, double bytes, hipStream_t stream) : s(stream), active(false), idx(0) {
    Profiler* p = g_prof;
    if (!p || !p->on) return;
    Profiler::Rec r{p->detailed ? std::string(kernel) + ":" + p->layer : std::string(kernel), flops, bytes, p->get(), p->get()};
    idx = p->recs.size();
    p->recs.push_back(r);
    active = true;
    (void)hipEventRecord(r.e0, s);
}
ProfScope::~ProfScope() {
    if (active && g_prof) (void)hipEventRecord(g_prof->recs[idx].e1, s);
}
}  // namespace ssd

using namespace ssd;

struct ssd_net {
    std::unique_ptr<Net> net;
};

#define API_BEGIN try {
#define API_END                                  \
    return 0;                                    \
    }                                            \
    catch (const std::exception& e) {            \
        ssd::set_error("%s", e.what());          \
        return 1;                                \
    }                                            \
    catch (...) {                                \
        ssd::set_error("unknown error");         \
        return 1;                                \
    }

static Net& N(ssd_handle h) {
    if (!h || !h->net) fail("null handle");
    return *h->net;
}
// handle-based entry points: the handle's GPU is current for the call, the caller's device is restored on return
#define API_BEGIN_NET(h) \
    try {                \
        Net& n = N(h);   \
        DeviceGuard dev_guard_(n.device());

// Label encoding is called once per training batch: the anchor tables of a (preset, device) pair and a small
// growable scratch per device are kept for the life of the process instead of six hipMalloc / hipFree pairs
// (each one a device synchronisation) per call.
namespace {
struct EncodeCache {
    struct Anchors { double* anc = nullptr; int* aabs = nullptr; };
    struct Scratch { char* p = nullptr; size_t bytes = 0; };
    std::mutex mu;
    std::map<std::pair<std::string, int>, Anchors> anchors;
    std::map<int, Scratch> scratch;
};
EncodeCache& encode_cache() {
    static EncodeCache* c = new EncodeCache();      // leaked on purpose: no HIP calls in static destructors
    return *c;
}
}  // namespace

extern "C" {

const char* ssd_last_error(void) { return ssd::get_error(); }
const char* ssd_version(void) { return "ssdvgg_hip 0.1 gfx950 fp32-mfma(v_mfma_f32_32x32x2_f32) bf16-mfma(v_mfma_f32_32x32x16_bf16)"; }

int ssd_preset_info(const char* preset, int* image_w, int* image_h, int* num_anchors, int* num_maps) {
    API_BEGIN
    const Preset& p = get_preset(preset);
    if (image_w) *image_w = p.image_w;
    if (image_h) *image_h = p.image_h;
    if (num_anchors) *num_anchors = p.num_anchors;
    if (num_maps) *num_maps = p.nmaps;
    API_END
}

int ssd_preset_map(const char* preset, int map, int* size, double* scale, int* num_types) {
    API_BEGIN
    const Preset& p = get_preset(preset);
    SSD_REQUIRE(map >= 0 && map < p.nmaps, "map %d outside 0..%d", map, p.nmaps - 1);
    if (size) *size = p.map_size[map];
    if (scale) *scale = p.scale[map];
    if (num_types) *num_types = p.ntypes[map];
    API_END
}

int ssd_anchors_dev(const char* preset, double* anchors_dev, int* anchors_abs_dev, void* stream) {
    API_BEGIN
    anchors_device(get_preset(preset), anchors_dev, anchors_abs_dev, (hipStream_t)stream);
    API_END
}

static void anchors_host(const char* preset, int device, double* out, int* out_abs) {
    const Preset& p = get_preset(preset);
    DeviceGuard dev_guard_(device);
    const size_t A = p.num_anchors;
    DevBuf a(A * 4 * sizeof(double)), b(A * 4 * sizeof(int));
    anchors_device(p, a.as<double>(), b.as<int>(), nullptr);
    if (out) HIP_OK(hipMemcpy(out, a.p, A * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_abs) HIP_OK(hipMemcpy(out_abs, b.p, A * 4 * sizeof(int), hipMemcpyDeviceToHost));
}

int ssd_anchors(const char* preset, int device, double* out) {
    API_BEGIN
    anchors_host(preset, device, out, nullptr);
    API_END
}

int ssd_anchors_abs(const char* preset, int device, int* out) {
    API_BEGIN
    anchors_host(preset, device, nullptr, out);
    API_END
}

int ssd_jaccard_overlap(int device, const double* box, const double* boxes, int n, double* iou_out) {
    API_BEGIN
    SSD_REQUIRE(n >= 0, "n must be >= 0");
    if (n > 0) {
        DeviceGuard dev_guard_(device);
        DevBuf db(4 * sizeof(double)), da((size_t)n * 4 * sizeof(double)), di((size_t)n * sizeof(double));
        HIP_OK(hipMemcpy(db.p, box, 4 * sizeof(double), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(da.p, boxes, (size_t)n * 4 * sizeof(double), hipMemcpyHostToDevice));
        jaccard_device(db.as<double>(), da.as<double>(), n, di.as<double>(), nullptr);
        HIP_OK(hipMemcpy(iou_out, di.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    }
    API_END
}

// the preset's anchor tables on `device`, built once (caller holds ec.mu)
static EncodeCache::Anchors& encode_anchors(EncodeCache& ec, const Preset& p, int device) {
    const size_t A = p.num_anchors;
    EncodeCache::Anchors& an = ec.anchors[{p.name, device}];
    if (!an.anc) {
        // built into locals and published only once complete: a failure half way must not leave a table that looks ready
        double* anc = nullptr;
        int* aabs = nullptr;
        try {
            HIP_OK(hipMalloc((void**)&anc, A * 4 * sizeof(double)));
            HIP_OK(hipMalloc((void**)&aabs, A * 4 * sizeof(int)));
            anchors_device(p, anc, aabs, nullptr);
            HIP_OK(hipDeviceSynchronize());
        } catch (...) {
            if (anc) (void)hipFree(anc);
            if (aabs) (void)hipFree(aabs);
            throw;
        }
        an.aabs = aabs;
        an.anc = anc;
    }
    return an;
}

// match_dev / match_host: where the [b*A] winning-box indices go (at most one of the two; both null: not wanted)
static void encode_labels_impl(const char* preset, int num_classes, int device, const double* gt, const int* cls,
                               const int* offsets, int b, float* vec_dev, float* vec_host, hipStream_t s,
                               int match = MATCH_REFERENCE, int* match_dev = nullptr, int* match_host = nullptr) {
    require_match(match);                // before any HIP call
    const Preset& p = get_preset(preset);
    SSD_REQUIRE(b >= 1, "batch must be >= 1");
    require_num_classes(num_classes);
    DeviceGuard dev_guard_(device);
    const int ntot = offsets[b];
    SSD_REQUIRE(offsets[0] == 0 && ntot >= 0, "gt_offsets must start at 0 and be non-decreasing");
    for (int i = 0; i < ntot; ++i)
        SSD_REQUIRE(cls[i] >= 0 && cls[i] < num_classes, "gt_cls[%d] = %d outside 0..%d", i, cls[i], num_classes - 1);
    const size_t A = p.num_anchors;
    EncodeCache& ec = encode_cache();
    std::lock_guard<std::mutex> lock(ec.mu);
    EncodeCache::Anchors& an = encode_anchors(ec, p, device);
    const size_t nt = ntot ? ntot : 1;
    const size_t n = (size_t)b * A * (num_classes + 5);
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t o_gt = 0, o_cls = o_gt + up(nt * 4 * sizeof(double)), o_off = o_cls + up(nt * sizeof(int)),
                 o_ws = o_off + up((size_t)(b + 1) * sizeof(int)), o_tmp = o_ws + up(encode_labels_ws_bytes_ex(ntot, b, match)),
                 o_match = o_tmp + up(vec_dev ? 0 : n * sizeof(float)),
                 need = o_match + (match_host ? (size_t)b * A * sizeof(int) : 0);
    EncodeCache::Scratch& sc = ec.scratch[device];
    if (need > sc.bytes) {
        if (sc.p) HIP_OK(hipFree(sc.p));
        sc.p = nullptr; sc.bytes = 0;
        HIP_OK(hipMalloc((void**)&sc.p, need));
        sc.bytes = need;
    }
    double* dgt = (double*)(sc.p + o_gt);
    int* dcls = (int*)(sc.p + o_cls);
    int* doff = (int*)(sc.p + o_off);
    float* out = vec_dev ? vec_dev : (float*)(sc.p + o_tmp);
    int* mout = match_host ? (int*)(sc.p + o_match) : match_dev;
    try {
        if (ntot) {
            HIP_OK(hipMemcpyAsync(dgt, gt, (size_t)ntot * 4 * sizeof(double), hipMemcpyHostToDevice, s));
            HIP_OK(hipMemcpyAsync(dcls, cls, (size_t)ntot * sizeof(int), hipMemcpyHostToDevice, s));
        }
        HIP_OK(hipMemcpyAsync(doff, offsets, (size_t)(b + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        encode_labels_ex(p, num_classes, an.anc, an.aabs, dgt, dcls, doff, b, ntot, out, mout, match, sc.p + o_ws, s);
        if (vec_host) HIP_OK(hipMemcpyAsync(vec_host, out, n * sizeof(float), hipMemcpyDeviceToHost, s));
        if (match_host) HIP_OK(hipMemcpyAsync(match_host, mout, (size_t)b * A * sizeof(int), hipMemcpyDeviceToHost, s));
    } catch (...) {
        (void)hipStreamSynchronize(s);   // nothing of this call may still be using the shared scratch when the lock is released
        throw;
    }
    HIP_OK(hipStreamSynchronize(s));     // the shared scratch is free for the next call
}

int ssd_encode_labels(const char* preset, int num_classes, int device, const double* gt_boxes, const int* gt_cls,
                      const int* gt_offsets, int b, float* vec_out) {
    API_BEGIN
    encode_labels_impl(preset, num_classes, device, gt_boxes, gt_cls, gt_offsets, b, nullptr, vec_out, nullptr);
    API_END
}

int ssd_encode_labels_dev(const char* preset, int num_classes, int device, const double* gt_boxes, const int* gt_cls,
                          const int* gt_offsets, int b, float* vec_out_dev, void* stream) {
    API_BEGIN
    encode_labels_impl(preset, num_classes, device, gt_boxes, gt_cls, gt_offsets, b, vec_out_dev, nullptr, (hipStream_t)stream);
    API_END
}

int ssd_encode_labels_ex(const char* preset, int num_classes, int device, const double* gt_boxes, const int* gt_cls,
                         const int* gt_offsets, int b, float* vec_out, int match, int* match_out) {
    API_BEGIN
    encode_labels_impl(preset, num_classes, device, gt_boxes, gt_cls, gt_offsets, b, nullptr, vec_out, nullptr, match, nullptr, match_out);
    API_END
}

int ssd_encode_labels_dev_ex(const char* preset, int num_classes, int device, const double* gt_boxes, const int* gt_cls,
                             const int* gt_offsets, int b, float* vec_out_dev, void* stream, int match, int* match_out_dev) {
    API_BEGIN
    encode_labels_impl(preset, num_classes, device, gt_boxes, gt_cls, gt_offsets, b, vec_out_dev, nullptr, (hipStream_t)stream, match,
                       match_out_dev, nullptr);
    API_END
}

size_t ssd_encode_labels_ws_bytes(int ntot) { return (encode_labels_ws_bytes(ntot) + 255) / 256 * 256; }

size_t ssd_encode_labels_ws_bytes_ex(int ntot, int b, int match) {
    try {
        return (encode_labels_ws_bytes_ex(ntot, b, match) + 255) / 256 * 256;
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_encode_labels_resident(const char* preset, int num_classes, int device, const double* gt_boxes_dev, const int* gt_cls_dev,
                               const int* gt_offsets_dev, int b, int ntot, float* vec_out_dev, void* ws_dev, void* stream) {
    return ssd_encode_labels_resident_ex(preset, num_classes, device, gt_boxes_dev, gt_cls_dev, gt_offsets_dev, b, ntot, vec_out_dev,
                                         ws_dev, stream, SSD_MATCH_REFERENCE, nullptr);
}

int ssd_encode_labels_resident_ex(const char* preset, int num_classes, int device, const double* gt_boxes_dev, const int* gt_cls_dev,
                                  const int* gt_offsets_dev, int b, int ntot, float* vec_out_dev, void* ws_dev, void* stream,
                                  int match, int* match_out_dev) {
    API_BEGIN
    require_match(match);                // before any HIP call
    const Preset& p = get_preset(preset);
    SSD_REQUIRE(b >= 1 && ntot >= 0, "batch must be >= 1 and ntot >= 0");
    require_num_classes(num_classes);
    SSD_REQUIRE(gt_offsets_dev && vec_out_dev && ws_dev && (ntot == 0 || (gt_boxes_dev && gt_cls_dev)), "null argument");
    DeviceGuard dev_guard_(device);
    const double* anc;
    const int* aabs;
    {
        EncodeCache& ec = encode_cache();
        std::lock_guard<std::mutex> lock(ec.mu);
        EncodeCache::Anchors& an = encode_anchors(ec, p, device);
        anc = an.anc; aabs = an.aabs;
    }
    encode_labels_ex(p, num_classes, anc, aabs, gt_boxes_dev, gt_cls_dev, gt_offsets_dev, b, ntot, vec_out_dev, match_out_dev, match, ws_dev,
                     (hipStream_t)stream);
    API_END
}

size_t ssd_decode_nms_ws_bytes(const char* preset, int b) {
    try {
        return detect_ws_bytes(b, get_preset(preset).num_anchors);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_decode_nms_dev(const char* preset, int num_classes, const double* anchors_dev, const float* pred_dev, int b,
                       float conf_thr, int cap, int max_out, int out_cap, int nms, int* count_dev, float* conf_dev,
                       int* cls_dev, int* idx_dev, int* box_dev, void* ws_dev, void* stream) {
    API_BEGIN
    const Preset& p = get_preset(preset);
    DetectOut o{count_dev, conf_dev, cls_dev, idx_dev, box_dev};
    detect(p.num_anchors, num_classes, anchors_dev, pred_dev, b, conf_thr, cap, max_out, out_cap, nms != 0, o, ws_dev,
           (hipStream_t)stream);
    API_END
}

int ssd_decode_nms(const char* preset, int num_classes, int device, const float* pred, int b, float conf_thr, int cap,
                   int max_out, int out_cap, int nms, int* count, float* conf, int* cls, int* idx, int* box) {
    API_BEGIN
    require_num_classes(num_classes);
    const Preset& p = get_preset(preset);
    SSD_REQUIRE(b >= 1 && out_cap >= 1, "batch and out_cap must be >= 1");
    DeviceGuard dev_guard_(device);
    const size_t A = p.num_anchors, nv = num_classes + 5, n = (size_t)b * out_cap;
    DevBuf anc(A * 4 * sizeof(double)), dpred((size_t)b * A * nv * sizeof(float)), ws(detect_ws_bytes(b, (int)A));
    DevBuf dcount((size_t)b * 4), dconf(n * 4), dcls(n * 4), didx(n * 4), dbox(n * 16);
    anchors_device(p, anc.as<double>(), nullptr, nullptr);
    HIP_OK(hipMemcpy(dpred.p, pred, (size_t)b * A * nv * sizeof(float), hipMemcpyHostToDevice));
    DetectOut o{dcount.as<int>(), dconf.as<float>(), dcls.as<int>(), didx.as<int>(), dbox.as<int>()};
    detect((int)A, num_classes, anc.as<double>(), dpred.as<float>(), b, conf_thr, cap, max_out, out_cap, nms != 0, o, ws.p, nullptr);
    HIP_OK(hipMemcpy(count, dcount.p, (size_t)b * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(conf, dconf.p, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(cls, dcls.p, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(idx, didx.p, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(box, dbox.p, n * 16, hipMemcpyDeviceToHost));
    API_END
}

size_t ssd_detection_output_ws_bytes(const char* preset, int num_classes, int b, int nms_top_k) {
    try {
        detection_output_check(get_preset(preset).num_anchors, num_classes, b, 0.f, nms_top_k, 1, 1);
        return detection_output_ws_bytes(b, num_classes, nms_top_k);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_detection_output_dev(const char* preset, int num_classes, const double* anchors_dev, const float* pred_dev, int b,
                             float conf_thr, int nms_top_k, int keep_top_k, int out_cap, int* count_dev, float* conf_dev,
                             int* cls_dev, int* idx_dev, int* box_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    API_BEGIN
    const Preset& p = get_preset(preset);
    DetectOut o{count_dev, conf_dev, cls_dev, idx_dev, box_dev};
    detection_output(p.num_anchors, num_classes, anchors_dev, pred_dev, b, conf_thr, nms_top_k, keep_top_k, out_cap, o, ws_dev,
                     ws_bytes, (hipStream_t)stream);
    API_END
}

int ssd_detection_output(const char* preset, int num_classes, int device, const float* pred, int b, float conf_thr,
                         int nms_top_k, int keep_top_k, int out_cap, int* count, float* conf, int* cls, int* idx, int* box) {
    API_BEGIN
    const Preset& p = get_preset(preset);
    detection_output_check(p.num_anchors, num_classes, b, conf_thr, nms_top_k, keep_top_k, out_cap);
    SSD_REQUIRE(pred && count && conf && cls && idx && box, "null argument");
    DeviceGuard dev_guard_(device);
    const size_t A = p.num_anchors, nv = num_classes + 5, n = (size_t)b * out_cap;
    const size_t wsb = detection_output_ws_bytes(b, num_classes, nms_top_k);
    DevBuf anc(A * 4 * sizeof(double)), dpred((size_t)b * A * nv * sizeof(float)), ws(wsb);
    DevBuf dcount((size_t)b * 4), dconf(n * 4), dcls(n * 4), didx(n * 4), dbox(n * 16);
    anchors_device(p, anc.as<double>(), nullptr, nullptr);
    HIP_OK(hipMemcpy(dpred.p, pred, (size_t)b * A * nv * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dconf.p, 0, n * 4));       // rows past an image's count read as zero
    HIP_OK(hipMemset(dcls.p, 0, n * 4));
    HIP_OK(hipMemset(didx.p, 0, n * 4));
    HIP_OK(hipMemset(dbox.p, 0, n * 16));
    DetectOut o{dcount.as<int>(), dconf.as<float>(), dcls.as<int>(), didx.as<int>(), dbox.as<int>()};
    detection_output((int)A, num_classes, anc.as<double>(), dpred.as<float>(), b, conf_thr, nms_top_k, keep_top_k, out_cap, o, ws.p, wsb,
                     nullptr);
    HIP_OK(hipMemcpy(count, dcount.p, (size_t)b * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(conf, dconf.p, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(cls, dcls.p, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(idx, didx.p, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(box, dbox.p, n * 16, hipMemcpyDeviceToHost));
    API_END
}

static_assert(sizeof(ssd_nms_params) == sizeof(NmsParams) && SSD_NMS_HARD == NMS_HARD && SSD_NMS_SOFT_LINEAR == NMS_SOFT_LINEAR &&
                  SSD_NMS_SOFT_GAUSSIAN == NMS_SOFT_GAUSSIAN,
              "ssd_nms_params is boxes.h's NmsParams");

// the parameters of a *_soft entry point, refused before anything else is looked at
static NmsParams soft_params(const char* who, const ssd_nms_params* nms) {
    nms_params_check(who, reinterpret_cast<const NmsParams*>(nms));
    return *reinterpret_cast<const NmsParams*>(nms);
}

int ssd_detection_output_soft_dev(const char* preset, int num_classes, const double* anchors_dev, const float* pred_dev, int b,
                                  float conf_thr, int nms_top_k, int keep_top_k, int out_cap, int* count_dev, float* conf_dev,
                                  int* cls_dev, int* idx_dev, int* box_dev, void* ws_dev, size_t ws_bytes, const ssd_nms_params* nms,
                                  void* stream) {
    API_BEGIN
    const NmsParams np = soft_params("ssd_detection_output_soft_dev", nms);
    const Preset& p = get_preset(preset);
    DetectOut o{count_dev, conf_dev, cls_dev, idx_dev, box_dev};
    detection_output(p.num_anchors, num_classes, anchors_dev, pred_dev, b, conf_thr, nms_top_k, keep_top_k, out_cap, o, ws_dev,
                     ws_bytes, (hipStream_t)stream, np);
    API_END
}

int ssd_detection_output_soft(const char* preset, int num_classes, int device, const float* pred, int b, float conf_thr,
                              int nms_top_k, int keep_top_k, int out_cap, int* count, float* conf, int* cls, int* idx, int* box,
                              const ssd_nms_params* nms) {
    API_BEGIN
    const NmsParams np = soft_params("ssd_detection_output_soft", nms);
    const Preset& p = get_preset(preset);
    detection_output_check(p.num_anchors, num_classes, b, conf_thr, nms_top_k, keep_top_k, out_cap);
    SSD_REQUIRE(pred && count && conf && cls && idx && box, "null argument");
    DeviceGuard dev_guard_(device);
    const size_t A = p.num_anchors, nv = num_classes + 5, n = (size_t)b * out_cap;
    const size_t wsb = detection_output_ws_bytes(b, num_classes, nms_top_k);
    DevBuf anc(A * 4 * sizeof(double)), dpred((size_t)b * A * nv * sizeof(float)), ws(wsb);
    DevBuf dcount((size_t)b * 4), dconf(n * 4), dcls(n * 4), didx(n * 4), dbox(n * 16);
    anchors_device(p, anc.as<double>(), nullptr, nullptr);
    HIP_OK(hipMemcpy(dpred.p, pred, (size_t)b * A * nv * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dconf.p, 0, n * 4));       // rows past an image's count read as zero
    HIP_OK(hipMemset(dcls.p, 0, n * 4));
    HIP_OK(hipMemset(didx.p, 0, n * 4));
    HIP_OK(hipMemset(dbox.p, 0, n * 16));
    DetectOut o{dcount.as<int>(), dconf.as<float>(), dcls.as<int>(), didx.as<int>(), dbox.as<int>()};
    detection_output((int)A, num_classes, anc.as<double>(), dpred.as<float>(), b, conf_thr, nms_top_k, keep_top_k, out_cap, o, ws.p, wsb,
                     nullptr, np);
    HIP_OK(hipMemcpy(count, dcount.p, (size_t)b * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(conf, dconf.p, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(cls, dcls.p, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(idx, didx.p, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(box, dbox.p, n * 16, hipMemcpyDeviceToHost));
    API_END
}

int ssd_soft_nms_boxes(int device, int n, const int* box_abs, const float* conf, const ssd_nms_params* nms, int* order_out,
                       float* conf_out, int* n_keep) {
    API_BEGIN
    const char* who = "ssd_soft_nms_boxes";
    const NmsParams np = soft_params(who, nms);
    SSD_REQUIRE(np.kind != NMS_HARD, "%s: nms kind must be 1 (soft, linear) or 2 (soft, gaussian): the hard rule on a list is ssd_nms_boxes", who);
    SSD_REQUIRE(n >= 0 && n <= 1024, "%s: 0..1024 boxes (got %d)", who, n);
    SSD_REQUIRE(n_keep != nullptr, "%s: n_keep is null", who);
    *n_keep = 0;
    if (n > 0) {
        SSD_REQUIRE(box_abs && conf && order_out && conf_out, "%s: null argument", who);
        for (int i = 0; i < n; ++i) {
            const int* bx = box_abs + (size_t)i * 4;
            SSD_REQUIRE(bx[0] >= 0 && bx[0] <= bx[1] && bx[1] <= 999 && bx[2] >= 0 && bx[2] <= bx[3] && bx[3] <= 999,
                        "%s: box %d (%d, %d, %d, %d) is not xmin <= xmax, ymin <= ymax on the 1000 grid", who, i, bx[0], bx[1], bx[2], bx[3]);
            SSD_REQUIRE(std::isfinite(conf[i]) && !std::signbit(conf[i]), "%s: conf[%d] must be finite and non-negative", who, i);
        }
        DeviceGuard dev_guard_(device);
        DevBuf dbox((size_t)n * 16), dconf((size_t)n * 4), dorder((size_t)n * 4), dout((size_t)n * 4), dkeep(4);
        HIP_OK(hipMemcpy(dbox.p, box_abs, (size_t)n * 16, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dconf.p, conf, (size_t)n * 4, hipMemcpyHostToDevice));
        soft_nms_boxes_device(n, dbox.as<int>(), dconf.as<float>(), np, dorder.as<int>(), dout.as<float>(), dkeep.as<int>(), nullptr);
        int keep = 0;
        HIP_OK(hipMemcpy(&keep, dkeep.p, 4, hipMemcpyDeviceToHost));
        SSD_REQUIRE(keep >= 0 && keep <= n, "%s: the kernel reported %d picks of %d boxes", who, keep, n);
        if (keep > 0) {
            HIP_OK(hipMemcpy(order_out, dorder.p, (size_t)keep * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(conf_out, dout.p, (size_t)keep * 4, hipMemcpyDeviceToHost));
        }
        *n_keep = keep;
    }
    API_END
}

int ssd_nms_boxes(int device, int n, const int* box_abs, const float* conf, const int* group, double iou_thr, int* keep_out,
                  int* n_keep) {
    API_BEGIN
    SSD_REQUIRE(n >= 0 && n <= 65535, "ssd_nms_boxes: 0..65535 boxes (got %d)", n);
    SSD_REQUIRE(n_keep != nullptr, "n_keep is null");
    *n_keep = 0;
    if (n > 0) {
        SSD_REQUIRE(box_abs && conf && keep_out, "null argument");
        int ngroups = 1;
        if (group)
            for (int i = 0; i < n; ++i) {
                SSD_REQUIRE(group[i] >= 0 && group[i] < 65535, "group[%d] = %d outside 0..65534", i, group[i]);
                ngroups = std::max(ngroups, group[i] + 1);
            }
        DeviceGuard dev_guard_(device);
        DevBuf dbox((size_t)n * 16), dconf((size_t)n * 4), dgrp((size_t)n * 4), dkeep((size_t)n * 4 + 4), ws(nms_boxes_ws_bytes(n, ngroups));
        HIP_OK(hipMemcpy(dbox.p, box_abs, (size_t)n * 16, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dconf.p, conf, (size_t)n * 4, hipMemcpyHostToDevice));
        if (group) HIP_OK(hipMemcpy(dgrp.p, group, (size_t)n * 4, hipMemcpyHostToDevice));
        else HIP_OK(hipMemset(dgrp.p, 0, (size_t)n * 4));
        nms_boxes_device(n, ngroups, dbox.as<int>(), dconf.as<float>(), dgrp.as<int>(), iou_thr, dkeep.as<int>(), ws.p, nullptr);
        std::vector<int> tmp((size_t)n + 1);
        HIP_OK(hipMemcpy(tmp.data(), dkeep.p, (size_t)n * 4 + 4, hipMemcpyDeviceToHost));
        *n_keep = tmp[0];
        for (int i = 0; i < tmp[0]; ++i) keep_out[i] = tmp[1 + i];
    }
    API_END
}

static_assert(sizeof(ssd_tile) == sizeof(MergeTile), "ssd_tile is boxes.h's MergeTile");

int ssd_merge_tiles_limits(int* max_tiles, int* max_candidates, int* lds_keys) {
    API_BEGIN
    if (max_tiles) *max_tiles = MERGE_MAX_TILES;
    if (max_candidates) *max_candidates = MERGE_MAX_CAND;
    if (lds_keys) *lds_keys = MERGE_LDS_KEYS;
    API_END
}

size_t ssd_merge_tiles_ws_bytes(int n_tiles, int tile_cap) {
    try {
        return merge_tiles_ws_bytes(n_tiles, tile_cap);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_merge_tiles_dev(const ssd_tile* tiles, int n_tiles, int n_images, int tile_cap, const int* count_dev, const float* conf_dev,
                        const int* cls_dev, const int* idx_dev, const int* box_dev, int edge_margin, int max_out, int out_cap,
                        int* count_out, float* conf_out, int* cls_out, int* idx_out, int* tile_out, int* box_out, void* ws_dev,
                        void* stream) {
    API_BEGIN
    merge_tiles(reinterpret_cast<const MergeTile*>(tiles), n_tiles, n_images, tile_cap, count_dev, conf_dev, cls_dev, idx_dev, box_dev,
                edge_margin, max_out, out_cap, count_out, conf_out, cls_out, idx_out, tile_out, box_out, ws_dev, (hipStream_t)stream);
    API_END
}

int ssd_merge_tiles(int device, const ssd_tile* tiles, int n_tiles, int n_images, int tile_cap, const int* count, const float* conf,
                    const int* cls, const int* idx, const int* box, int edge_margin, int max_out, int out_cap, int* count_out,
                    float* conf_out, int* cls_out, int* idx_out, int* tile_out, int* box_out) {
    API_BEGIN
    SSD_REQUIRE(tiles && count && conf && cls && idx && box && count_out && cls_out && box_out, "ssd_merge_tiles: null argument");
    merge_tiles_check(reinterpret_cast<const MergeTile*>(tiles), n_tiles, n_images, tile_cap, out_cap);
    const size_t ws_bytes = merge_tiles_ws_bytes(n_tiles, tile_cap);
    for (int t = 0; t < n_tiles; ++t)
        for (int j = 0; j < std::min(count[t], tile_cap); ++j) {
            const int c = cls[(size_t)t * tile_cap + j];
            SSD_REQUIRE(c >= 0 && c < MAX_CLASSES, "ssd_merge_tiles: tile %d, record %d: class id %d outside 0..%d", t, j, c,
                        MAX_CLASSES - 1);
        }
    DeviceGuard dev_guard_(device);
    const size_t nin = (size_t)n_tiles * tile_cap, nout = (size_t)n_images * out_cap;
    DevBuf dcount((size_t)n_tiles * 4), dconf(nin * 4), dcls(nin * 4), didx(nin * 4), dbox(nin * 16), ws(ws_bytes);
    DevBuf ocount((size_t)n_images * 4), oconf(nout * 4), ocls(nout * 4), oidx(nout * 4), otile(nout * 4), obox(nout * 16);
    HIP_OK(hipMemcpy(dcount.p, count, (size_t)n_tiles * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dconf.p, conf, nin * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dcls.p, cls, nin * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(didx.p, idx, nin * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dbox.p, box, nin * 16, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(oconf.p, 0, nout * 4));
    HIP_OK(hipMemset(ocls.p, 0, nout * 4));
    HIP_OK(hipMemset(oidx.p, 0, nout * 4));
    HIP_OK(hipMemset(otile.p, 0, nout * 4));
    HIP_OK(hipMemset(obox.p, 0, nout * 16));
    merge_tiles(reinterpret_cast<const MergeTile*>(tiles), n_tiles, n_images, tile_cap, dcount.as<int>(), dconf.as<float>(),
                dcls.as<int>(), didx.as<int>(), dbox.as<int>(), edge_margin, max_out, out_cap, ocount.as<int>(), oconf.as<float>(),
                ocls.as<int>(), oidx.as<int>(), otile.as<int>(), obox.as<int>(), ws.p, nullptr);
    HIP_OK(hipMemcpy(count_out, ocount.p, (size_t)n_images * 4, hipMemcpyDeviceToHost));
    if (conf_out) HIP_OK(hipMemcpy(conf_out, oconf.p, nout * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(cls_out, ocls.p, nout * 4, hipMemcpyDeviceToHost));
    if (idx_out) HIP_OK(hipMemcpy(idx_out, oidx.p, nout * 4, hipMemcpyDeviceToHost));
    if (tile_out) HIP_OK(hipMemcpy(tile_out, otile.p, nout * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(box_out, obox.p, nout * 16, hipMemcpyDeviceToHost));
    API_END
}

size_t ssd_detout_tiles_ws_bytes(const char* preset, int num_classes, int n_tiles, int n_images, int nms_top_k) {
    try {
        return detout_tiles_ws_bytes(get_preset(preset).num_anchors, num_classes, n_tiles, n_images, nms_top_k);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_detout_tiles_add_dev(const char* preset, int num_classes, const double* anchors_dev, const float* pred_dev,
                             const ssd_tile* tiles, int n_tiles, int first, int b, float conf_thr, int nms_top_k, int edge_margin,
                             void* ws_dev, size_t ws_bytes, void* stream) {
    API_BEGIN
    detout_tiles_add("ssd_detout_tiles_add_dev", get_preset(preset).num_anchors, num_classes, anchors_dev, pred_dev,
                     reinterpret_cast<const MergeTile*>(tiles), n_tiles, first, b, conf_thr, nms_top_k, edge_margin, ws_dev, ws_bytes,
                     (hipStream_t)stream);
    API_END
}

int ssd_detout_tiles_merge_dev(int num_classes, const ssd_tile* tiles, int n_tiles, int n_images, int nms_top_k, int keep_top_k,
                               int out_cap, int* count_out, float* conf_out, int* cls_out, int* idx_out, int* tile_out, int* box_out,
                               void* ws_dev, size_t ws_bytes, void* stream) {
    API_BEGIN
    detout_tiles_merge("ssd_detout_tiles_merge_dev", num_classes, reinterpret_cast<const MergeTile*>(tiles), n_tiles, n_images, nms_top_k,
                       keep_top_k, out_cap, count_out, conf_out, cls_out, idx_out, tile_out, box_out, ws_dev, ws_bytes,
                       (hipStream_t)stream);
    API_END
}

int ssd_detout_tiles_merge_soft_dev(int num_classes, const ssd_tile* tiles, int n_tiles, int n_images, int nms_top_k, int keep_top_k,
                                    int out_cap, int* count_out, float* conf_out, int* cls_out, int* idx_out, int* tile_out,
                                    int* box_out, void* ws_dev, size_t ws_bytes, const ssd_nms_params* nms, void* stream) {
    API_BEGIN
    const char* who = "ssd_detout_tiles_merge_soft_dev";
    const NmsParams np = soft_params(who, nms);
    detout_tiles_merge(who, num_classes, reinterpret_cast<const MergeTile*>(tiles), n_tiles, n_images, nms_top_k, keep_top_k, out_cap,
                       count_out, conf_out, cls_out, idx_out, tile_out, box_out, ws_dev, ws_bytes, (hipStream_t)stream, np);
    API_END
}

static int detout_tiles_host(const char* who, const NmsParams& np, const char* preset, int num_classes, int device, const float* pred,
                             const ssd_tile* tiles, int n_tiles, int n_images, float conf_thr, int nms_top_k, int keep_top_k,
                             int edge_margin, int out_cap, int* count_out, float* conf_out, int* cls_out, int* idx_out, int* tile_out,
                             int* box_out);

int ssd_detout_tiles_soft(const char* preset, int num_classes, int device, const float* pred, const ssd_tile* tiles, int n_tiles,
                          int n_images, float conf_thr, int nms_top_k, int keep_top_k, int edge_margin, int out_cap, int* count_out,
                          float* conf_out, int* cls_out, int* idx_out, int* tile_out, int* box_out, const ssd_nms_params* nms) {
    API_BEGIN
    const char* who = "ssd_detout_tiles_soft";
    const NmsParams np = soft_params(who, nms);
    return detout_tiles_host(who, np, preset, num_classes, device, pred, tiles, n_tiles, n_images, conf_thr, nms_top_k, keep_top_k,
                             edge_margin, out_cap, count_out, conf_out, cls_out, idx_out, tile_out, box_out);
    API_END
}

int ssd_detout_tiles(const char* preset, int num_classes, int device, const float* pred, const ssd_tile* tiles, int n_tiles,
                     int n_images, float conf_thr, int nms_top_k, int keep_top_k, int edge_margin, int out_cap, int* count_out,
                     float* conf_out, int* cls_out, int* idx_out, int* tile_out, int* box_out) {
    return detout_tiles_host("ssd_detout_tiles", NmsParams{NMS_HARD, 0.f, 0.f, 0.f}, preset, num_classes, device, pred, tiles, n_tiles,
                             n_images, conf_thr, nms_top_k, keep_top_k, edge_margin, out_cap, count_out, conf_out, cls_out, idx_out,
                             tile_out, box_out);
}

static int detout_tiles_host(const char* who, const NmsParams& np, const char* preset, int num_classes, int device, const float* pred,
                             const ssd_tile* tiles, int n_tiles, int n_images, float conf_thr, int nms_top_k, int keep_top_k,
                             int edge_margin, int out_cap, int* count_out, float* conf_out, int* cls_out, int* idx_out, int* tile_out,
                             int* box_out) {
    API_BEGIN
    const Preset& p = get_preset(preset);
    const MergeTile* mt = reinterpret_cast<const MergeTile*>(tiles);
    {      // every limit before anything is allocated
        std::vector<int> head;
        detout_tiles_add_check(who, p.num_anchors, num_classes, mt, n_tiles, 0, n_tiles, conf_thr, nms_top_k, head);
        detout_tiles_merge_check(who, num_classes, mt, n_tiles, n_images, nms_top_k, keep_top_k, out_cap, head);
    }
    SSD_REQUIRE(pred && count_out && cls_out && box_out, "%s: null argument", who);
    DeviceGuard dev_guard_(device);
    const size_t A = p.num_anchors, nv = num_classes + 5, nout = (size_t)n_images * out_cap;
    const size_t wsb = detout_tiles_ws_bytes((int)A, num_classes, n_tiles, n_images, nms_top_k);
    DevBuf anc(A * 4 * sizeof(double)), dpred((size_t)n_tiles * A * nv * sizeof(float)), ws(wsb);
    DevBuf ocount((size_t)n_images * 4), oconf(nout * 4), ocls(nout * 4), oidx(nout * 4), otile(nout * 4), obox(nout * 16);
    anchors_device(p, anc.as<double>(), nullptr, nullptr);
    HIP_OK(hipMemcpy(dpred.p, pred, (size_t)n_tiles * A * nv * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(oconf.p, 0, nout * 4));      // rows past a picture's count read as zero
    HIP_OK(hipMemset(ocls.p, 0, nout * 4));
    HIP_OK(hipMemset(oidx.p, 0, nout * 4));
    HIP_OK(hipMemset(otile.p, 0, nout * 4));
    HIP_OK(hipMemset(obox.p, 0, nout * 16));
    detout_tiles_add(who, (int)A, num_classes, anc.as<double>(), dpred.as<float>(), mt, n_tiles, 0, n_tiles, conf_thr, nms_top_k,
                     edge_margin, ws.p, wsb, nullptr);
    detout_tiles_merge(who, num_classes, mt, n_tiles, n_images, nms_top_k, keep_top_k, out_cap, ocount.as<int>(), oconf.as<float>(),
                       ocls.as<int>(), oidx.as<int>(), otile.as<int>(), obox.as<int>(), ws.p, wsb, nullptr, np);
    HIP_OK(hipMemcpy(count_out, ocount.p, (size_t)n_images * 4, hipMemcpyDeviceToHost));
    if (conf_out) HIP_OK(hipMemcpy(conf_out, oconf.p, nout * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(cls_out, ocls.p, nout * 4, hipMemcpyDeviceToHost));
    if (idx_out) HIP_OK(hipMemcpy(idx_out, oidx.p, nout * 4, hipMemcpyDeviceToHost));
    if (tile_out) HIP_OK(hipMemcpy(tile_out, otile.p, nout * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(box_out, obox.p, nout * 16, hipMemcpyDeviceToHost));
    API_END
}

int ssd_average_precision_ex(int device, int n_det, const float* det_box, const float* det_conf, const int* det_cls,
                             const int* det_sample, int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample,
                             const unsigned char* gt_flags, int num_classes, int protocol, int n_thr, const double* minoverlaps,
                             double* ap_out, int* present_out) {
    API_BEGIN
    SSD_REQUIRE(num_classes >= 1 && n_det >= 0 && n_gt >= 0, "bad sizes");
    for (int g = 1; g < n_gt; ++g) SSD_REQUIRE(gt_sample[g] >= gt_sample[g - 1], "ground truth must be grouped by ascending sample id");
    DeviceGuard dev_guard_(device);
    const size_t nd = n_det ? n_det : 1, ng = n_gt ? n_gt : 1;
    DevBuf dbox(nd * 16), dconf(nd * 4), dcls(nd * 4), dsmp(nd * 4), gbox(ng * 32), gcls(ng * 4), gsmp(ng * 4), gflg(ng);
    if (n_det) {
        HIP_OK(hipMemcpy(dbox.p, det_box, nd * 16, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dconf.p, det_conf, nd * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dcls.p, det_cls, nd * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dsmp.p, det_sample, nd * 4, hipMemcpyHostToDevice));
    }
    if (n_gt) {
        HIP_OK(hipMemcpy(gbox.p, gt_box, ng * 32, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(gcls.p, gt_cls, ng * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(gsmp.p, gt_sample, ng * 4, hipMemcpyHostToDevice));
    }
    if (n_gt && gt_flags) HIP_OK(hipMemcpy(gflg.p, gt_flags, ng, hipMemcpyHostToDevice));
    else HIP_OK(hipMemset(gflg.p, 0, ng));
    APInput in{n_det, n_gt, num_classes, dbox.as<float>(), dconf.as<float>(), dcls.as<int>(), dsmp.as<int>(), gbox.as<double>(),
               gcls.as<int>(), gsmp.as<int>(), gflg.as<unsigned char>()};
    average_precision_run(in, protocol, n_thr, minoverlaps, ap_out, present_out, nullptr);
    API_END
}

int ssd_average_precision(int device, int n_det, const float* det_box, const float* det_conf, const int* det_cls,
                          const int* det_sample, int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample,
                          int num_classes, double minoverlap, double* ap_out, int* present_out) {
    return ssd_average_precision_ex(device, n_det, det_box, det_conf, det_cls, det_sample, n_gt, gt_box, gt_cls, gt_sample, nullptr,
                                    num_classes, AP_REFERENCE, 1, &minoverlap, ap_out, present_out);
}

static_assert(SSD_AP_REFERENCE == AP_REFERENCE && SSD_AP_VOC07 == AP_VOC07 && SSD_AP_VOC12 == AP_VOC12, "protocol ids");

static APAccumulator& ACC(ssd_ap_accumulator a) {
    if (!a) fail("null accumulator");
    return *reinterpret_cast<APAccumulator*>(a);
}

int ssd_ap_create(int device, int num_classes, ssd_ap_accumulator* acc) {
    API_BEGIN
    SSD_REQUIRE(acc, "ssd_ap_create: null argument");
    *acc = reinterpret_cast<ssd_ap_accumulator>(new APAccumulator(device, num_classes));
    API_END
}

int ssd_ap_destroy(ssd_ap_accumulator acc) {
    API_BEGIN
    delete reinterpret_cast<APAccumulator*>(acc);
    API_END
}

int ssd_ap_clear(ssd_ap_accumulator acc) {
    API_BEGIN
    ACC(acc).clear();
    API_END
}

int ssd_ap_add_dev(ssd_ap_accumulator acc, int b, int out_cap, const int* count_dev, const float* conf_dev, const int* cls_dev,
                   const int* box_dev, int n_gt, const double* gt_box, const int* gt_cls, const int* gt_image,
                   const unsigned char* gt_flags, void* stream) {
    API_BEGIN
    ACC(acc).add_dev(b, out_cap, count_dev, conf_dev, cls_dev, box_dev, n_gt, gt_box, gt_cls, gt_image, gt_flags, (hipStream_t)stream);
    API_END
}

int ssd_ap_add_host(ssd_ap_accumulator acc, int n_det, const float* det_box, const float* det_conf, const int* det_cls,
                    const int* det_sample, int n_samples, int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample,
                    const unsigned char* gt_flags) {
    API_BEGIN
    ACC(acc).add_host(n_det, det_box, det_conf, det_cls, det_sample, n_samples, n_gt, gt_box, gt_cls, gt_sample, gt_flags);
    API_END
}

int ssd_ap_count(ssd_ap_accumulator acc, long long* n_det, long long* n_dropped) {
    API_BEGIN
    ACC(acc).counts(n_det, n_dropped);
    API_END
}

int ssd_ap_fetch(ssd_ap_accumulator acc, long long cap, float* det_box, float* det_conf, int* det_cls, int* det_sample,
                 long long* n_det) {
    API_BEGIN
    ACC(acc).fetch(cap, det_box, det_conf, det_cls, det_sample, n_det);
    API_END
}

int ssd_ap_compute(ssd_ap_accumulator acc, int protocol, int n_thr, const double* minoverlaps, double* ap_out, int* present_out,
                   long long* n_det, long long* n_dropped) {
    API_BEGIN
    ACC(acc).compute(protocol, n_thr, minoverlaps, ap_out, present_out, n_det, n_dropped);
    API_END
}

int ssd_coco_eval(int device, int n_det, const float* det_box, const float* det_conf, const int* det_cls, const int* det_sample,
                  int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample, const unsigned char* gt_flags,
                  const double* gt_area, int n_samples, const double* sample_scale, int num_classes, int n_thr,
                  const double* thresholds, double* ap_out, double* ar_out, int* present_out) {
    API_BEGIN
    SSD_REQUIRE(num_classes >= 1 && n_det >= 0 && n_gt >= 0 && n_samples >= 0, "ssd_coco_eval: bad sizes");
    SSD_REQUIRE(n_thr >= 1 && n_thr <= AP_MAX_THRESHOLDS && thresholds, "ssd_coco_eval: 1..%d IoU thresholds (got %d)", AP_MAX_THRESHOLDS, n_thr);
    SSD_REQUIRE(ap_out && ar_out && present_out, "ssd_coco_eval: null output array");
    SSD_REQUIRE(n_det == 0 || (det_box && det_conf && det_cls && det_sample), "ssd_coco_eval: null detection array");
    SSD_REQUIRE(n_gt == 0 || (gt_box && gt_cls && gt_sample && gt_area), "ssd_coco_eval: null ground-truth array");
    SSD_REQUIRE(n_samples == 0 || sample_scale, "ssd_coco_eval: null sample_scale");
    for (int i = 0; i < n_samples; ++i)
        SSD_REQUIRE(sample_scale[i] > 0.0, "ssd_coco_eval: sample_scale[%d] = %g must be positive (W*H/1e6 of the image)", i, sample_scale[i]);
    for (int g = 0; g < n_gt; ++g) {
        SSD_REQUIRE(g == 0 || gt_sample[g] >= gt_sample[g - 1], "ssd_coco_eval: ground truth must be grouped by ascending sample id");
        SSD_REQUIRE(gt_sample[g] >= 0 && gt_sample[g] < n_samples, "ssd_coco_eval: ground truth %d belongs to sample %d outside 0..%d", g, gt_sample[g], n_samples - 1);
        SSD_REQUIRE(gt_cls[g] >= 0 && gt_cls[g] < num_classes, "ssd_coco_eval: ground truth %d has class id %d outside 0..%d", g, gt_cls[g], num_classes - 1);
        SSD_REQUIRE(gt_area[g] >= 0.0, "ssd_coco_eval: gt_area[%d] = %g is negative", g, gt_area[g]);
    }
    for (int d = 0; d < n_det; ++d) {
        SSD_REQUIRE(det_sample[d] >= 0 && det_sample[d] < n_samples, "ssd_coco_eval: detection %d belongs to sample %d outside 0..%d", d, det_sample[d], n_samples - 1);
        SSD_REQUIRE(det_cls[d] >= 0 && det_cls[d] < num_classes, "ssd_coco_eval: detection %d has class id %d outside 0..%d", d, det_cls[d], num_classes - 1);
    }
    DeviceGuard dev_guard_(device);
    const size_t nd = n_det ? n_det : 1, ng = n_gt ? n_gt : 1, ns = n_samples ? n_samples : 1;
    DevBuf dbox(nd * 16), dconf(nd * 4), dcls(nd * 4), dsmp(nd * 4), gbox(ng * 32), gcls(ng * 4), gsmp(ng * 4), gflg(ng), garea(ng * 8),
        scale(ns * 8);
    if (n_det) {
        HIP_OK(hipMemcpy(dbox.p, det_box, nd * 16, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dconf.p, det_conf, nd * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dcls.p, det_cls, nd * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dsmp.p, det_sample, nd * 4, hipMemcpyHostToDevice));
    }
    if (n_gt) {
        HIP_OK(hipMemcpy(gbox.p, gt_box, ng * 32, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(gcls.p, gt_cls, ng * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(gsmp.p, gt_sample, ng * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(garea.p, gt_area, ng * 8, hipMemcpyHostToDevice));
    }
    if (n_gt && gt_flags) HIP_OK(hipMemcpy(gflg.p, gt_flags, ng, hipMemcpyHostToDevice));
    else HIP_OK(hipMemset(gflg.p, 0, ng));
    if (n_samples) HIP_OK(hipMemcpy(scale.p, sample_scale, ns * 8, hipMemcpyHostToDevice));
    COCOInput c{{n_det, n_gt, num_classes, dbox.as<float>(), dconf.as<float>(), dcls.as<int>(), dsmp.as<int>(), gbox.as<double>(),
                 gcls.as<int>(), gsmp.as<int>(), gflg.as<unsigned char>()}, n_samples, garea.as<double>(), scale.as<double>(), nullptr};
    coco_eval_run(c, gt_sample, n_thr, thresholds, ap_out, ar_out, present_out, nullptr);
    API_END
}

int ssd_ap_add_dev_coco(ssd_ap_accumulator acc, int b, int out_cap, const int* count_dev, const float* conf_dev, const int* cls_dev,
                        const int* box_dev, int n_gt, const double* gt_box, const int* gt_cls, const int* gt_image,
                        const unsigned char* gt_flags, const double* gt_area, const double* sample_scale, void* stream) {
    API_BEGIN
    SSD_REQUIRE(sample_scale, "ssd_ap_add_dev_coco: null sample_scale");
    ACC(acc).add_dev_coco(b, out_cap, count_dev, conf_dev, cls_dev, box_dev, n_gt, gt_box, gt_cls, gt_image, gt_flags, gt_area, sample_scale,
                          (hipStream_t)stream);
    API_END
}

int ssd_ap_add_host_coco(ssd_ap_accumulator acc, int n_det, const float* det_box, const float* det_conf, const int* det_cls,
                         const int* det_sample, int n_samples, int n_gt, const double* gt_box, const int* gt_cls, const int* gt_sample,
                         const unsigned char* gt_flags, const double* gt_area, const double* sample_scale) {
    API_BEGIN
    SSD_REQUIRE(sample_scale || n_samples == 0, "ssd_ap_add_host_coco: null sample_scale");
    static const double none = 1.0;      // (no samples: the pass still counts as one with scales)
    ACC(acc).add_host_coco(n_det, det_box, det_conf, det_cls, det_sample, n_samples, n_gt, gt_box, gt_cls, gt_sample, gt_flags, gt_area,
                           sample_scale ? sample_scale : &none);
    API_END
}

int ssd_ap_compute_coco(ssd_ap_accumulator acc, int n_thr, const double* thresholds, double* ap_out, double* ar_out, int* present_out,
                        long long* n_det, long long* n_dropped) {
    API_BEGIN
    ACC(acc).compute_coco(n_thr, thresholds, ap_out, ar_out, present_out, n_det, n_dropped);
    API_END
}

int ssd_ap_kernel_times(int enable, double* ms_out) {
    API_BEGIN
    ap_kernel_times(enable, ms_out);
    API_END
}

// ------------------------------------------------------------------------------ model
size_t ssd_arena_floats(const char* preset, int num_classes) {
    try {
        return Net::arena_floats(preset, num_classes);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

size_t ssd_arena_floats_graph(const char* preset, int num_classes, int graph) {
    try {
        return Net::arena_floats(preset, num_classes, graph);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_jpeg_info(const unsigned char* bytes, size_t n, int* width, int* height, int* components, int* sampling, int* status) {
    if (status) *status = SSD_JPEG_ERROR;
    API_BEGIN
    SSD_REQUIRE(status != nullptr, "status is null");
    ssd_jpeg_desc d;
    const int st = jpeg_parse_header(bytes, n, &d);
    if (width) *width = d.width;
    if (height) *height = d.height;
    if (components) *components = d.components;
    if (sampling) *sampling = d.hs * 16 + d.vs;
    *status = st;
    API_END
}

size_t ssd_jpeg_coef_bytes(const unsigned char* bytes, size_t n) {
    try {
        ssd_jpeg_desc d;
        return jpeg_parse_header(bytes, n, &d) == SSD_JPEG_OK ? jpeg_coef_bytes(d) : 0;
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_jpeg_entropy_decode(const unsigned char* bytes, size_t n, short* coef_out, size_t coef_cap_bytes, ssd_jpeg_desc* desc,
                            int* status) {
    if (status) *status = SSD_JPEG_ERROR;
    API_BEGIN
    SSD_REQUIRE(status != nullptr && desc != nullptr, "null argument");
    *status = jpeg_entropy_decode(bytes, n, coef_out, coef_cap_bytes, desc);
    API_END
}

int ssd_jpeg_entropy_decode_batch(const unsigned char* const* files, const size_t* sizes, int n, int threads, short* coef_out,
                                  const unsigned long long* offsets, ssd_jpeg_desc* descs, int* status_out) {
    API_BEGIN
    jpeg_entropy_decode_batch(files, sizes, n, threads, coef_out, offsets, descs, status_out);
    API_END
}

size_t ssd_jpeg_ws_bytes(const ssd_jpeg_desc* descs, int n) {
    try {
        return jpeg_ws_bytes(descs, n);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_jpeg_decode_batch_dev(const short* coef_dev, size_t coef_bytes, const ssd_jpeg_desc* descs, int n, unsigned char* dst_dev,
                              size_t dst_bytes, void* ws_dev, size_t ws_bytes, void* stream) {
    API_BEGIN
    jpeg_decode_batch(coef_dev, coef_bytes, descs, n, dst_dev, dst_bytes, ws_dev, ws_bytes, (hipStream_t)stream);
    API_END
}

size_t ssd_jpeg_scan_segments(const unsigned char* bytes, size_t n) {
    try {
        return jpeg_scan_segments(bytes, n);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_jpeg_scan_plan(const unsigned char* bytes, size_t n, ssd_jpeg_desc* desc, ssd_jpeg_plan* plan, int* status) {
    if (status) *status = SSD_JPEG_ERROR;
    API_BEGIN
    SSD_REQUIRE(status != nullptr && desc != nullptr && plan != nullptr, "null argument");
    *status = jpeg_scan_plan(bytes, n, desc, plan);
    API_END
}

size_t ssd_jpeg_huffdec_ws_bytes(const ssd_jpeg_plan* plans, const ssd_jpeg_desc* descs, int n) {
    try {
        return jpeg_huffdec_ws_bytes(plans, descs, n);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_jpeg_huffdec_batch_dev(const unsigned char* files_dev, size_t files_bytes, const ssd_jpeg_plan* plans,
                               const ssd_jpeg_desc* descs, int n, short* coef_dev, size_t coef_bytes, ssd_jpeg_huffdec_rec* recs_dev,
                               void* ws_dev, size_t ws_bytes, int max_rounds, void* stream) {
    API_BEGIN
    jpeg_huffdec_batch(files_dev, files_bytes, plans, descs, n, coef_dev, coef_bytes, recs_dev, ws_dev, ws_bytes, max_rounds, (hipStream_t)stream);
    API_END
}

int ssd_jpeg_quant_tables(int quality, unsigned short* luma, unsigned short* chroma) {
    API_BEGIN
    jpeg_quant_tables(quality, luma, chroma);
    API_END
}

size_t ssd_jpeg_enc_coef_bytes(const int* shapes, int n, int sampling) {
    try {
        return jpeg_enc_coef_bytes(shapes, n, sampling);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

size_t ssd_jpeg_enc_ws_bytes(const int* shapes, int n, int sampling) {
    try {
        return jpeg_enc_ws_bytes(shapes, n, sampling);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_jpeg_encode_batch_dev(const unsigned char* src_dev, size_t src_bytes, const unsigned long long* src_offs, const int* shapes,
                              int n, int quality, int sampling, short* coef_dev, size_t coef_bytes, ssd_jpeg_desc* descs_out,
                              void* ws_dev, size_t ws_bytes, void* stream) {
    API_BEGIN
    jpeg_encode_batch(src_dev, src_bytes, src_offs, shapes, n, quality, sampling, coef_dev, coef_bytes, descs_out, ws_dev, ws_bytes,
                      (hipStream_t)stream);
    API_END
}

size_t ssd_jpeg_file_bound(const ssd_jpeg_desc* desc) {
    try {
        SSD_REQUIRE(desc != nullptr, "null argument");
        return jpeg_file_bound(*desc);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_jpeg_entropy_encode(const short* coef, size_t coef_bytes, const ssd_jpeg_desc* desc, unsigned char* out, size_t out_cap,
                            size_t* out_size) {
    if (out_size) *out_size = 0;
    API_BEGIN
    SSD_REQUIRE(desc != nullptr && out_size != nullptr, "null argument");
    *out_size = jpeg_entropy_encode(coef, coef_bytes, *desc, out, out_cap);
    API_END
}

int ssd_jpeg_entropy_encode_batch(const short* coef, size_t coef_bytes, const ssd_jpeg_desc* descs, int n, int threads,
                                  unsigned char* out, size_t out_bytes, const unsigned long long* out_offsets,
                                  unsigned long long* out_sizes) {
    API_BEGIN
    jpeg_entropy_encode_batch(coef, coef_bytes, descs, n, threads, out, out_bytes, out_offsets, out_sizes);
    API_END
}

int ssd_jpeg_file_header(const ssd_jpeg_desc* desc, unsigned char* out) {
    API_BEGIN
    SSD_REQUIRE(desc != nullptr, "null argument");
    jpeg_file_header(*desc, out);
    API_END
}

size_t ssd_jpeg_huff_ws_bytes(const ssd_jpeg_desc* descs, int n) {
    try {
        return jpeg_huff_ws_bytes(descs, n);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

size_t ssd_jpeg_huff_out_bytes(const ssd_jpeg_desc* descs, int n) {
    try {
        return jpeg_huff_out_bytes(descs, n);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}

int ssd_jpeg_huffman_batch_dev(const short* coef_dev, size_t coef_bytes, const ssd_jpeg_desc* descs, int n, unsigned char* out_dev,
                               size_t out_bytes, ssd_jpeg_file_rec* files_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    API_BEGIN
    jpeg_huffman_batch(coef_dev, coef_bytes, descs, n, out_dev, out_bytes, files_dev, ws_dev, ws_bytes, (hipStream_t)stream);
    API_END
}

size_t ssd_augment_ws_bytes(int b, int out_w, int out_h) { return augment_ws_bytes(b, out_w, out_h); }

int ssd_augment_batch_dev(const unsigned char* images_dev, const ssd_augment_params* params, int b, int out_w, int out_h,
                          float* out_dev, void* ws_dev, void* stream) {
    API_BEGIN
    SSD_REQUIRE(images_dev && params && out_dev && ws_dev, "null argument");
    augment_batch(images_dev, params, b, out_w, out_h, out_dev, ws_dev, (hipStream_t)stream);
    API_END
}

size_t ssd_augment_cells_ws_bytes(int n_cells, int out_w, int out_h) { return augment_cells_ws_bytes(n_cells, out_w, out_h); }

int ssd_augment_cells_dev(const unsigned char* images_dev, const ssd_augment_params* params, const ssd_augment_cell* cells, int n_cells, int b,
                          int out_w, int out_h, float* out_dev, void* ws_dev, void* stream) {
    API_BEGIN
    SSD_REQUIRE(images_dev && params && cells && out_dev && ws_dev, "null argument");
    augment_cells(images_dev, params, cells, n_cells, b, out_w, out_h, out_dev, ws_dev, (hipStream_t)stream);
    API_END
}

// ---------------------------------------------------------------------------------- drawing
struct ssd_annotate_style_s {
    ssd::AnnotateStyle* style;
};

int ssd_annotate_rect(const int box1000[4], int w, int h, int out[4]) {
    API_BEGIN
    annotate_rect(box1000, w, h, out);
    API_END
}

int ssd_annotate_glyph(int ch, unsigned char rows[7]) {
    API_BEGIN
    annotate_glyph(ch, rows);
    API_END
}

int ssd_annotate_style_create(int device, int num_classes, const unsigned char* colors_bgr, const char* names, ssd_annotate_style* out) {
    API_BEGIN
    SSD_REQUIRE(out != nullptr, "out style pointer is null");
    *out = nullptr;
    require_num_classes(num_classes);
    DeviceGuard dev_guard_(device);
    std::unique_ptr<AnnotateStyle, void (*)(AnnotateStyle*)> st(annotate_style_create(device, num_classes, colors_bgr, names), annotate_style_destroy);
    *out = new ssd_annotate_style_s{st.get()};
    st.release();
    API_END
}

int ssd_annotate_style_destroy(ssd_annotate_style s) {
    API_BEGIN
    if (s) {
        annotate_style_destroy(s->style);
        delete s;
    }
    API_END
}

size_t ssd_annotate_ws_bytes(int b, int out_cap) { return annotate_ws_bytes(b, out_cap); }

int ssd_annotate_batch_dev(const void* src_dev, int src_is_f32, const ssd_annotate_image* images, int b, const int* count_dev,
                           const int* cls_dev, const int* box_dev, int out_cap, int boxes_on_1000_grid, ssd_annotate_style style,
                           int rgb_out, void* dst_dev, int dst_is_f32, void* ws_dev, void* stream) {
    API_BEGIN
    SSD_REQUIRE(style && style->style, "annotate: null style");
    DeviceGuard dev_guard_(annotate_style_device(style->style));
    annotate_batch(src_dev, src_is_f32 != 0, images, b, count_dev, cls_dev, box_dev, out_cap, boxes_on_1000_grid != 0, style->style,
                   rgb_out != 0, dst_dev, dst_is_f32 != 0, ws_dev, (hipStream_t)stream);
    API_END
}

static int create_handle(const char* preset, int num_classes, int max_batch, int device, int training, unsigned long long seed,
                         float* ext_params_dev, float* ext_grads_dev, float* ext_momentum_dev, int dtype, int graph, ssd_handle* out) {
    API_BEGIN
    SSD_REQUIRE(out != nullptr, "out handle pointer is null");
    *out = nullptr;
    SSD_REQUIRE(!(dtype == SSD_DTYPE_FP8 && training), "SSD_DTYPE_FP8 is inference only: create the handle with training = 0");
    SSD_REQUIRE(!(dtype == SSD_DTYPE_MXFP8 && training), "SSD_DTYPE_MXFP8 is inference only: create the handle with training = 0");
    SSD_REQUIRE(!(dtype == SSD_DTYPE_MXFP6 && training), "SSD_DTYPE_MXFP6 is inference only: create the handle with training = 0");
    DeviceGuard dev_guard_(device);
    auto n = std::make_unique<Net>(preset, num_classes, max_batch, device, training != 0, seed, ext_params_dev, ext_grads_dev,
                                   ext_momentum_dev, dtype, graph);
    SSD_REQUIRE(n->nparams() == Net::arena_floats(preset, num_classes, graph), "arena size mismatch");
    *out = new ssd_net{std::move(n)};
    API_END
}

int ssd_create(const char* preset, int num_classes, int max_batch, int device, int training, unsigned long long seed,
               float* ext_params_dev, float* ext_grads_dev, float* ext_momentum_dev, ssd_handle* out) {
    return create_handle(preset, num_classes, max_batch, device, training, seed, ext_params_dev, ext_grads_dev, ext_momentum_dev, 0, 0, out);
}

int ssd_create_dtype(const char* preset, int num_classes, int max_batch, int device, int training, unsigned long long seed,
                     float* ext_params_dev, float* ext_grads_dev, float* ext_momentum_dev, int dtype, ssd_handle* out) {
    return create_handle(preset, num_classes, max_batch, device, training, seed, ext_params_dev, ext_grads_dev, ext_momentum_dev, dtype, 0, out);
}

int ssd_create_graph(const char* preset, int num_classes, int max_batch, int device, int training, unsigned long long seed,
                     float* ext_params_dev, float* ext_grads_dev, float* ext_momentum_dev, int dtype, int graph, ssd_handle* out) {
    return create_handle(preset, num_classes, max_batch, device, training, seed, ext_params_dev, ext_grads_dev, ext_momentum_dev, dtype, graph, out);
}

int ssd_graph(ssd_handle h, int* graph) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(h != nullptr && graph != nullptr, "null argument");
    *graph = n.graph();
    API_END
}

int ssd_get_dtype(ssd_handle h, int* dtype) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(h != nullptr && dtype != nullptr, "null argument");
    *dtype = n.dtype();
    API_END
}

int ssd_destroy(ssd_handle h) {
    API_BEGIN
    delete h;
    API_END
}

int ssd_set_stream(ssd_handle h, void* stream) {
    API_BEGIN_NET(h)
    n.set_stream((hipStream_t)stream);
    API_END
}

int ssd_num_variables(ssd_handle h) {
    try {
        return (int)N(h).variables().size();
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return -1;
    }
}

int ssd_variable_info(ssd_handle h, int i, char* name, int name_cap, int* ndim, int shape[4]) {
    API_BEGIN_NET(h)
    const auto& vars = n.variables();
    SSD_REQUIRE(i >= 0 && i < (int)vars.size(), "variable index %d outside 0..%zu", i, vars.size() - 1);
    const Variable& v = vars[i];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", v.name.c_str());
    if (ndim) *ndim = v.ndim;
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = v.shape[k];
    API_END
}

int ssd_load_variable(ssd_handle h, const char* name, const float* data, size_t count) {
    API_BEGIN_NET(h)
    n.load_variable(name, data, count, 0);
    API_END
}
int ssd_save_variable(ssd_handle h, const char* name, float* data, size_t count) {
    API_BEGIN_NET(h)
    n.save_variable(name, data, count, 0);
    API_END
}
int ssd_save_gradient(ssd_handle h, const char* name, float* data, size_t count) {
    API_BEGIN_NET(h)
    n.save_variable(name, data, count, 1);
    API_END
}
int ssd_save_momentum(ssd_handle h, const char* name, float* data, size_t count) {
    API_BEGIN_NET(h)
    n.save_variable(name, data, count, 2);
    API_END
}
int ssd_load_momentum(ssd_handle h, const char* name, const float* data, size_t count) {
    API_BEGIN_NET(h)
    n.load_variable(name, data, count, 2);
    API_END
}

int ssd_set_optimizer(ssd_handle h, const float* lr_values, const long long* lr_boundaries, int n_values, float momentum,
                      float weight_decay) {
    API_BEGIN_NET(h)
    n.set_optimizer(lr_values, lr_boundaries, n_values, momentum, weight_decay);
    API_END
}
int ssd_get_global_step(ssd_handle h, long long* step) {
    API_BEGIN_NET(h)
    *step = n.global_step;
    API_END
}
int ssd_set_global_step(ssd_handle h, long long step) {
    API_BEGIN_NET(h)
    n.global_step = step;
    API_END
}

int ssd_forward_backward_dev(ssd_handle h, const float* x_dev, const float* y_dev, int b) {
    API_BEGIN_NET(h)
    n.forward(x_dev, b, true, y_dev);
    n.backward(b, y_dev);
    API_END
}
int ssd_forward_dev(ssd_handle h, const float* x_dev, const float* y_dev, int b) {
    API_BEGIN_NET(h)
    n.forward(x_dev, b, true, y_dev);
    API_END
}
int ssd_backward_begin_dev(ssd_handle h, const float* y_dev, int b) {
    API_BEGIN_NET(h)
    n.backward_begin(b, y_dev);
    API_END
}
int ssd_backward_next_dev(ssd_handle h, size_t min_floats, int sync_main, size_t* offset, size_t* count, int* more) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(offset && count && more, "null output pointer");
    *more = n.backward_step(min_floats, offset, count, sync_main != 0) ? 1 : 0;
    API_END
}
int ssd_backward_ranges(ssd_handle h, size_t min_floats, size_t* offsets, size_t* counts, int cap, int* n_out) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(n_out != nullptr, "null argument");
    const auto r = n.backward_ranges(min_floats);
    *n_out = (int)r.size();
    for (int i = 0; i < (int)r.size() && i < cap; ++i) {
        if (offsets) offsets[i] = r[i].first;
        if (counts) counts[i] = r[i].second;
    }
    API_END
}
int ssd_set_wgrad_stream(ssd_handle h, void* stream) {
    API_BEGIN_NET(h)
    n.set_wgrad_stream((hipStream_t)stream);
    API_END
}
int ssd_apply_gradients_dev(ssd_handle h, float grad_scale) {
    API_BEGIN_NET(h)
    n.apply_gradients(grad_scale);
    API_END
}
int ssd_set_loss_normalizer(ssd_handle h, float batch) {
    API_BEGIN_NET(h)
    n.set_loss_normalizer(batch);
    API_END
}
// a loss configuration as the ABI takes it: refused here, on the host, before any HIP call (NULL means mining)
static void check_loss_config(const ssd_loss_config* cfg) {
    if (!cfg) return;
    SSD_REQUIRE(cfg->kind == SSD_LOSS_MINING || cfg->kind == SSD_LOSS_FOCAL, "loss: kind %d is neither SSD_LOSS_MINING nor SSD_LOSS_FOCAL",
                cfg->kind);
    if (cfg->kind != SSD_LOSS_FOCAL) return;
    SSD_REQUIRE(cfg->focal_gamma >= 0.f && cfg->focal_gamma <= 5.f, "loss: focal gamma %g outside [0, 5]", (double)cfg->focal_gamma);
    SSD_REQUIRE(cfg->focal_alpha > 0.f && cfg->focal_alpha < 1.f, "loss: focal alpha %g outside (0, 1)", (double)cfg->focal_alpha);
}
int ssd_set_loss(ssd_handle h, const ssd_loss_config* cfg) {
    API_BEGIN
    SSD_REQUIRE(cfg != nullptr, "loss: null configuration");
    check_loss_config(cfg);
    Net& n = N(h);
    SSD_REQUIRE(n.training(), "loss: the handle was created with training = 0");
    if (cfg->kind == SSD_LOSS_FOCAL) n.set_loss(cfg->kind, cfg->focal_gamma, cfg->focal_alpha);
    else n.set_loss(SSD_LOSS_MINING, 2.f, 0.25f);
    API_END
}
int ssd_get_loss(ssd_handle h, ssd_loss_config* cfg) {
    API_BEGIN
    SSD_REQUIRE(cfg != nullptr, "loss: null configuration");
    N(h).get_loss(&cfg->kind, &cfg->focal_gamma, &cfg->focal_alpha);
    API_END
}
// ... and a localization loss configuration (NULL means smooth-L1)
static void check_loc_loss_config(const ssd_loc_loss_config* cfg) {
    if (!cfg) return;
    SSD_REQUIRE(cfg->kind == SSD_LOC_SMOOTH_L1 || cfg->kind == SSD_LOC_GIOU,
                "localization loss: kind %d is neither SSD_LOC_SMOOTH_L1 nor SSD_LOC_GIOU", cfg->kind);
    if (cfg->kind != SSD_LOC_GIOU) return;
    SSD_REQUIRE(std::isfinite(cfg->weight) && cfg->weight > 0.f, "localization loss: weight %g is not a finite number > 0",
                (double)cfg->weight);
}
int ssd_set_loc_loss(ssd_handle h, const ssd_loc_loss_config* cfg) {
    API_BEGIN
    SSD_REQUIRE(cfg != nullptr, "localization loss: null configuration");
    check_loc_loss_config(cfg);
    Net& n = N(h);
    SSD_REQUIRE(n.training(), "localization loss: the handle was created with training = 0");
    if (cfg->kind == SSD_LOC_GIOU) n.set_loc_loss(cfg->kind, cfg->weight);
    else n.set_loc_loss(SSD_LOC_SMOOTH_L1, 1.f);
    API_END
}
int ssd_get_loc_loss(ssd_handle h, ssd_loc_loss_config* cfg) {
    API_BEGIN
    SSD_REQUIRE(cfg != nullptr, "localization loss: null configuration");
    N(h).get_loc_loss(&cfg->kind, &cfg->weight);
    API_END
}
// ... and a gradient clipping configuration: 0 off, a number > 0, or +inf (measure only)
static void check_grad_clip(float max_norm) {
    SSD_REQUIRE(max_norm >= 0.f, "gradient clipping: max_norm %g is neither 0 (off), a number > 0 nor +inf", (double)max_norm);
}
int ssd_set_grad_clip(ssd_handle h, const ssd_grad_clip_config* cfg) {
    API_BEGIN
    SSD_REQUIRE(cfg != nullptr, "gradient clipping: null configuration");
    check_grad_clip(cfg->max_norm);
    Net& n = N(h);
    n.set_grad_clip(cfg->max_norm == 0.f ? 0.f : cfg->max_norm);      // (-0 is stored as 0)
    API_END
}
int ssd_get_grad_clip(ssd_handle h, ssd_grad_clip_config* cfg) {
    API_BEGIN
    SSD_REQUIRE(cfg != nullptr, "gradient clipping: null configuration");
    cfg->max_norm = N(h).grad_clip();
    API_END
}
int ssd_get_grad_norm_step(ssd_handle h, int steps_back, float out[2]) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(out != nullptr, "null argument");
    n.get_grad_norm_step(steps_back, out);
    API_END
}
// ... and an update rule: the hyper-parameters in the order beta1, beta2, eps, decay (ops.h adamw_check), then the kind
static_assert(SSD_UPDATE_MOMENTUM == ssd::UPDATE_MOMENTUM && SSD_UPDATE_ADAMW == ssd::UPDATE_ADAMW, "ops.h mirrors the ABI's kinds");
int ssd_set_update_rule(ssd_handle h, const ssd_update_rule_config* cfg) {
    API_BEGIN
    SSD_REQUIRE(cfg != nullptr, "update rule: null configuration");
    adamw_check(cfg->beta1, cfg->beta2, cfg->eps, cfg->decay);
    SSD_REQUIRE(cfg->kind == SSD_UPDATE_MOMENTUM || cfg->kind == SSD_UPDATE_ADAMW,
                "update rule: kind %d is neither SSD_UPDATE_MOMENTUM nor SSD_UPDATE_ADAMW", cfg->kind);
    Net& n = N(h);
    DeviceGuard dev_guard_(n.device());
    n.set_update_rule(cfg->kind, cfg->beta1, cfg->beta2, cfg->eps, cfg->decay == 0.f ? 0.f : cfg->decay);
    API_END
}
int ssd_get_update_rule(ssd_handle h, ssd_update_rule_config* cfg) {
    API_BEGIN
    SSD_REQUIRE(cfg != nullptr, "update rule: null configuration");
    N(h).get_update_rule(&cfg->kind, &cfg->beta1, &cfg->beta2, &cfg->eps, &cfg->decay);
    API_END
}
int ssd_get_adam_step(ssd_handle h, long long* t) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(t != nullptr, "null argument");
    *t = n.adam_step();
    API_END
}
int ssd_set_adam_step(ssd_handle h, long long t) {
    API_BEGIN_NET(h)
    n.set_adam_step(t);
    API_END
}
int ssd_save_second_moment(ssd_handle h, const char* name, float* data, size_t count) {
    API_BEGIN_NET(h)
    n.save_variable(name, data, count, 3);
    API_END
}
int ssd_load_second_moment(ssd_handle h, const char* name, const float* data, size_t count) {
    API_BEGIN_NET(h)
    n.load_variable(name, data, count, 3);
    API_END
}
// ... and a weight EMA behind every update: the values are checked before the handle, like the rule's
static void check_ema_step(long long t) { SSD_REQUIRE(t >= 0, "weight EMA: the count of EMA updates must be >= 0, got %lld", t); }
int ssd_set_ema(ssd_handle h, float decay) {
    API_BEGIN
    if (decay != 0.f) ema_check(decay);
    Net& n = N(h);
    DeviceGuard dev_guard_(n.device());
    n.set_ema(decay == 0.f ? 0.f : decay);      // (-0 is stored as 0)
    API_END
}
int ssd_get_ema(ssd_handle h, float* decay, long long* t, int* swapped) {
    API_BEGIN
    Net& n = N(h);
    if (decay) *decay = n.ema_decay();
    if (t) *t = n.ema_step();
    if (swapped) *swapped = n.ema_swapped() ? 1 : 0;
    API_END
}
int ssd_set_ema_step(ssd_handle h, long long t) {
    API_BEGIN
    check_ema_step(t);
    N(h).set_ema_step(t);
    API_END
}
int ssd_save_ema(ssd_handle h, const char* name, float* data, size_t count) {
    API_BEGIN_NET(h)
    n.save_variable(name, data, count, 4);
    API_END
}
int ssd_load_ema(ssd_handle h, const char* name, const float* data, size_t count) {
    API_BEGIN_NET(h)
    n.load_variable(name, data, count, 4);
    API_END
}
int ssd_ema_swap(ssd_handle h) {
    API_BEGIN_NET(h)
    n.ema_swap_arenas();
    API_END
}
int ssd_null_gradients_dev(ssd_handle h) {
    API_BEGIN_NET(h)
    n.null_gradients_step();
    API_END
}
int ssd_train_step_dev(ssd_handle h, const float* x_dev, const float* y_dev, int b) {
    API_BEGIN_NET(h)
    n.forward(x_dev, b, true, y_dev);
    n.backward_apply(b, y_dev, 1.f);
    API_END
}
int ssd_eval_step_dev(ssd_handle h, const float* x_dev, const float* y_dev, int b) {
    API_BEGIN_NET(h)
    n.forward(x_dev, b, true, y_dev);
    API_END
}
int ssd_infer_dev(ssd_handle h, const float* x_dev, int b) {
    API_BEGIN_NET(h)
    n.forward(x_dev, b, false, nullptr);
    API_END
}
// fp8 handle: activation scales (net.hip plan_fp8)
int ssd_fp8_calibrate_dev(ssd_handle h, const float* x_dev, int b, int accumulate) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(x_dev != nullptr, "null argument");
    n.fp8_calibrate(x_dev, b, accumulate != 0);
    API_END
}
int ssd_fp8_num_scales(ssd_handle h, int* count) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(count != nullptr, "null argument");
    *count = n.fp8_num_scales();
    API_END
}
int ssd_fp8_scale_name(ssd_handle h, int i, char* name, int name_cap) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(name != nullptr && name_cap > 0, "null argument");
    snprintf(name, name_cap, "%s", n.fp8_scale_name(i));
    API_END
}
int ssd_fp8_get_scales(ssd_handle h, float* scales, int count) {
    API_BEGIN_NET(h)
    n.fp8_get_scales(scales, count);
    API_END
}
int ssd_fp8_set_scales(ssd_handle h, const float* scales, int count) {
    API_BEGIN_NET(h)
    n.fp8_set_scales(scales, count);
    API_END
}
int ssd_result_dev(ssd_handle h, const float** result_dev) {
    API_BEGIN_NET(h)
    *result_dev = n.result();
    API_END
}
int ssd_set_result_dev(ssd_handle h, const float* pred_dev, int b) {
    API_BEGIN_NET(h)
    n.set_result(pred_dev, b);
    API_END
}
int ssd_get_result(ssd_handle h, int b, float* result_out) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(h != nullptr && result_out != nullptr, "null argument");
    SSD_REQUIRE(b >= 1 && b <= n.max_batch(), "batch %d outside 1..%d", b, n.max_batch());
    n.copy_result(result_out, b);
    API_END
}

int ssd_get_losses(ssd_handle h, float losses_out[4]) {
    API_BEGIN_NET(h)
    n.get_losses(losses_out);
    API_END
}
int ssd_get_losses_step(ssd_handle h, int steps_back, float losses_out[4]) {
    API_BEGIN_NET(h)
    SSD_REQUIRE(losses_out != nullptr, "null argument");
    n.get_losses_step(steps_back, losses_out);
    API_END
}
int ssd_arenas(ssd_handle h, float** params_dev, float** grads_dev, float** momentum_dev, size_t* floats,
               size_t* filter_floats) {
    API_BEGIN_NET(h)
    if (params_dev) *params_dev = n.params();
    if (grads_dev) *grads_dev = n.grads();
    if (momentum_dev) *momentum_dev = n.momentum();
    if (floats) *floats = n.nparams();
    if (filter_floats) *filter_floats = n.nfilters();
    API_END
}

int ssd_train_step(ssd_handle h, const float* x, const float* y, int b, float* result_out, float losses_out[4]) {
    API_BEGIN_NET(h)
    n.upload_xy(x, y, b);
    n.forward(n.x_stage(), b, true, n.y_stage());
    n.backward_apply(b, n.y_stage(), 1.f);
    if (result_out) n.copy_result(result_out, b);
    if (losses_out) n.get_losses(losses_out);
    HIP_OK(hipStreamSynchronize(n.stream()));
    API_END
}
int ssd_eval_step(ssd_handle h, const float* x, const float* y, int b, float* result_out, float losses_out[4]) {
    API_BEGIN_NET(h)
    n.upload_xy(x, y, b);
    n.forward(n.x_stage(), b, true, n.y_stage());
    if (result_out) n.copy_result(result_out, b);
    if (losses_out) n.get_losses(losses_out);
    HIP_OK(hipStreamSynchronize(n.stream()));
    API_END
}
int ssd_infer(ssd_handle h, const float* x, int b, float* result_out) {
    API_BEGIN_NET(h)
    n.upload_xy(x, nullptr, b);
    n.forward(n.x_stage(), b, false, nullptr);
    if (result_out) n.copy_result(result_out, b);
    HIP_OK(hipStreamSynchronize(n.stream()));
    API_END
}

int ssd_detect_last(ssd_handle h, int b, float conf_thr, int cap, int max_out, int out_cap, int nms, int* count, float* conf,
                    int* cls, int* idx, int* box) {
    API_BEGIN_NET(h)
    n.detect_last(b, conf_thr, cap, max_out, out_cap, nms != 0, count, conf, cls, idx, box);
    API_END
}

int ssd_detect_last_dev(ssd_handle h, int b, float conf_thr, int cap, int max_out, int out_cap, int nms, int** count_dev,
                        float** conf_dev, int** cls_dev, int** idx_dev, int** box_dev) {
    API_BEGIN_NET(h)
    DetectOut d{};
    n.detect_last_dev(b, conf_thr, cap, max_out, out_cap, nms != 0, &d);
    if (count_dev) *count_dev = d.count;
    if (conf_dev) *conf_dev = d.conf;
    if (cls_dev) *cls_dev = d.cls;
    if (idx_dev) *idx_dev = d.idx;
    if (box_dev) *box_dev = d.box;
    API_END
}

int ssd_detect_last_all_dev(ssd_handle h, int b, float conf_thr, int nms_top_k, int keep_top_k, int out_cap, int** count_dev,
                            float** conf_dev, int** cls_dev, int** idx_dev, int** box_dev) {
    API_BEGIN_NET(h)
    DetectOut d{};
    n.detect_last_all_dev(b, conf_thr, nms_top_k, keep_top_k, out_cap, &d);
    if (count_dev) *count_dev = d.count;
    if (conf_dev) *conf_dev = d.conf;
    if (cls_dev) *cls_dev = d.cls;
    if (idx_dev) *idx_dev = d.idx;
    if (box_dev) *box_dev = d.box;
    API_END
}

int ssd_detect_last_all_soft_dev(ssd_handle h, int b, float conf_thr, int nms_top_k, int keep_top_k, int out_cap, int** count_dev,
                                 float** conf_dev, int** cls_dev, int** idx_dev, int** box_dev, const ssd_nms_params* nms) {
    API_BEGIN_NET(h)
    const NmsParams np = soft_params("ssd_detect_last_all_soft_dev", nms);
    DetectOut d{};
    n.detect_last_all_dev(b, conf_thr, nms_top_k, keep_top_k, out_cap, &d, np);
    if (count_dev) *count_dev = d.count;
    if (conf_dev) *conf_dev = d.conf;
    if (cls_dev) *cls_dev = d.cls;
    if (idx_dev) *idx_dev = d.idx;
    if (box_dev) *box_dev = d.box;
    API_END
}

int ssd_detect_fetch(ssd_handle h, int which, int* count, float* conf, int* cls, int* idx, int* box) {
    API_BEGIN_NET(h)
    n.detect_fetch(which, count, conf, cls, idx, box);
    API_END
}

int ssd_detect_host(ssd_handle h, int which, const int** count, const float** conf, const int** cls, const int** idx,
                    const int** box, int* b, int* out_cap) {
    API_BEGIN_NET(h)
    DetectOut d;
    n.detect_host(which, &d, b, out_cap);
    if (count) *count = d.count;
    if (conf) *conf = d.conf;
    if (cls) *cls = d.cls;
    if (idx) *idx = d.idx;
    if (box) *box = d.box;
    API_END
}

int ssd_set_overlap(ssd_handle h, int on) {
    API_BEGIN_NET(h)
    n.set_overlap(on != 0);
    API_END
}

int ssd_set_wino_dual(ssd_handle h, int on) {
    API_BEGIN_NET(h)
    n.set_wino_dual(on);
    API_END
}

int ssd_profile_enable(ssd_handle h, int on) {
    API_BEGIN_NET(h)
    n.profiler().on = on != 0;
    n.profiler().detailed = on == 2;
    n.profiler().reset();
    API_END
}

// one line per kernel label: "label\tlaunches\ttotal_ms\ttotal_flops\ttotal_bytes\n"
int ssd_profile_report(ssd_handle h, char* buf, size_t cap) {
    API_BEGIN_NET(h)
    HIP_OK(hipStreamSynchronize(n.stream()));
    struct Agg { long long cnt = 0; double ms = 0, fl = 0, by = 0; };
    std::map<std::string, Agg> agg;
    for (const auto& r : n.profiler().recs) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, r.e0, r.e1));
        Agg& a = agg[r.kernel];
        a.cnt++; a.ms += ms; a.fl += r.flops; a.by += r.bytes;
    }
    std::string out;
    char line[384];
    for (const auto& kv : agg) {
        snprintf(line, sizeof line, "%s\t%lld\t%.6f\t%.6e\t%.6e\n", kv.first.c_str(), kv.second.cnt, kv.second.ms, kv.second.fl,
                 kv.second.by);
        out += line;
    }
    SSD_REQUIRE(buf && cap > out.size(), "report needs %zu bytes", out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    n.profiler().reset();
    API_END
}

int ssd_activation_shape(ssd_handle h, const char* name, int* height, int* width, int* channels) {
    API_BEGIN_NET(h)
    n.activation_shape(name, height, width, channels);
    API_END
}

int ssd_activation(ssd_handle h, const char* name, int b, float* out, size_t count) {
    API_BEGIN_NET(h)
    n.activation(name, b, out, count);
    API_END
}

// --------------------------------------------------------------------- single kernels
static ConvDesc mk(int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h,
                   int pad_w) {
    ConvDesc d;
    d.B = b; d.Hi = hi; d.Wi = wi; d.Ci = ci; d.Ho = ho; d.Wo = wo; d.Co = co;
    d.KH = kh; d.KW = kw; d.stride = stride; d.dil = dil; d.pad_h = pad_h; d.pad_w = pad_w;
    return d;
}

int ssd_op_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int b, int hi, int wi, int ci, int ho,
                      int wo, int co, int kh, int kw, int stride, int dil, int pad_h, int pad_w, int relu, void* stream) {
    API_BEGIN
    conv_fwd(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), x, w, bias, y, relu != 0, (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_dgrad(const float* dy, const float* w, float* dx, const float* mask, int accumulate, int b, int hi, int wi,
                        int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h, int pad_w,
                        void* stream) {
    API_BEGIN
    conv_dgrad(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), dy, w, dx, mask, accumulate != 0,
               (hipStream_t)stream);
    API_END
}
int ssd_op_cast_filter(const float* w, void* w_io_bf16, void* w_oi_bf16, int taps, int ci, int co, void* stream) {
    API_BEGIN
    FilterCastPlan plan;
    plan.add(0, taps, ci, co);
    cast_filters(plan, w, (bf16_t*)w_io_bf16, (bf16_t*)w_oi_bf16, (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_fwd_bf16(const void* x, const void* w_oi, const float* bias, void* y, int y_f32, int b, int hi, int wi, int ci,
                           int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h, int pad_w, int relu,
                           void* stream) {
    API_BEGIN
    conv_fwd_bf16(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), (const bf16_t*)x, (const bf16_t*)w_oi, bias, y,
                  y_f32 != 0, relu != 0, (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_dgrad_bf16(const void* dy, const void* w_io, void* dx, const void* mask, int accumulate, int b, int hi, int wi,
                             int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h, int pad_w,
                             void* stream) {
    API_BEGIN
    conv_dgrad_bf16(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), (const bf16_t*)dy, (const bf16_t*)w_io,
                    (bf16_t*)dx, (const bf16_t*)mask, accumulate != 0, (hipStream_t)stream);
    API_END
}
size_t ssd_op_conv2d_wgrad_bf16_ws_floats(int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride,
                                          int dil, int pad_h, int pad_w) {
    return conv_wgrad_bf16_ws_floats(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w));
}
int ssd_op_conv2d_wgrad_bf16(const void* x, const void* dy, float* dw, float* dbias, const float* w, float weight_decay,
                             float* ws, int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride,
                             int dil, int pad_h, int pad_w, void* stream) {
    API_BEGIN
    conv_wgrad_bf16(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), (const bf16_t*)x, (const bf16_t*)dy, dw,
                    dbias, w, weight_decay, ws, (hipStream_t)stream);
    API_END
}
// one stage as a chain launch (unit-parity entry points: the step packs its filters once per weight update); the packed filter and
// the stage table are the call's own, freed on return
static void tail_chain_op(TailStage t, const void* mirror, int b, const char* label, hipStream_t s) {
    int device = 0;
    HIP_OK(hipGetDevice(&device));
    HipOwner tmp(device);
    TailTables tables{tmp, {}};
    void* packed = tmp.mem(tail_chain_packed_elems(t.d, t.dgrad) * 2);
    const TailPackItem it{t.d, t.dgrad, mirror, packed};
    tail_chain_pack_filters(&it, 1, s);
    t.wgt_packed = packed;
    tail_chain_bf16(&t, 1, b, label, s, tables);
    HIP_OK(hipStreamSynchronize(s));
}
int ssd_op_conv2d_fwd_bf16_chain(const void* x, const void* w_oi, const float* bias, void* y, int y_f32, int b, int hi, int wi, int ci,
                                 int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h, int pad_w, int relu,
                                 void* stream) {
    API_BEGIN
    TailStage t{};
    t.d = mk(1, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w);
    t.dgrad = false; t.src = x; t.bias = bias; t.dst = y; t.relu = relu != 0; t.out_f32 = y_f32 != 0;
    tail_chain_op(t, w_oi, b, "tail_fwd_bf16", (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_dgrad_bf16_chain(const void* dy, const void* w_io, void* dx, const void* mask, int accumulate, int b, int hi, int wi,
                                   int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h, int pad_w,
                                   void* stream) {
    API_BEGIN
    TailStage t{};
    t.d = mk(1, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w);
    t.dgrad = true; t.src = dy; t.mask = mask; t.dst = dx; t.accum = accumulate != 0;
    tail_chain_op(t, w_io, b, "tail_dgrad_bf16", (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_wgrad_bf16_direct(const void* x, const void* dy, float* dw, float* dbias, const float* w, float weight_decay, int b,
                                    int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h,
                                    int pad_w, void* stream) {
    API_BEGIN
    WgradGroupItem it{};
    it.d = mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w);
    it.x = (const bf16_t*)x; it.dy = (const bf16_t*)dy; it.dw = dw; it.dbias = dbias; it.w = w;
    conv_wgrad_group_bf16(&it, 1, weight_decay, (hipStream_t)stream);
    API_END
}
// several stages / layers per launch, as the step issues them (the plan alone: host only)
static_assert(SSD_TAIL_ZERO_BYTES == TAIL_ZERO_BYTES && SSD_TAIL_LDS_MAX == TAIL_LDS_MAX && SSD_TAIL_MAX_TASKS == TAIL_PLAN_MAX_TASKS, "ssdvgg_hip.h");
static_assert(SSD_TF_RELU == TF_RELU && SSD_TF_ACCUM == TF_ACCUM && SSD_TF_OUT_F32 == TF_OUT_F32 && SSD_TF_LOAD_IN == TF_LOAD_IN &&
              SSD_TF_LOAD_OUT == TF_LOAD_OUT && SSD_TF_KTAIL == TF_KTAIL, "ssdvgg_hip.h");
static_assert(sizeof(ssd_tail_plan_stage) == sizeof(TailPlanStage), "ssd_tail_plan_stage is TailPlanStage");
static std::vector<TailStage> tail_stages_of(const ssd_tail_stage* stages, int nstages) {
    SSD_REQUIRE(stages != nullptr && nstages >= 1 && nstages <= 4096, "tail chain: no stage list (%d stages)", nstages);
    std::vector<TailStage> st(nstages);
    for (int i = 0; i < nstages; ++i) {
        const ssd_tail_stage& a = stages[i];
        TailStage& t = st[i];
        t = TailStage{};
        t.d = mk(1, a.hi, a.wi, a.ci, a.ho, a.wo, a.co, a.kh, a.kw, a.stride, a.dil, a.pad_h, a.pad_w);
        t.dgrad = a.dgrad != 0; t.src = a.src; t.wgt_packed = a.wgt; t.bias = a.bias; t.mask = a.mask; t.dst = a.dst;
        t.relu = a.relu != 0; t.accum = a.accum != 0; t.out_f32 = a.out_f32 != 0;
    }
    return st;
}
int ssd_op_tail_chain_plan(const ssd_tail_stage* stages, int nstages, ssd_tail_plan_stage* plan_out, int* lds_total_out) {
    API_BEGIN
    SSD_REQUIRE(plan_out != nullptr && lds_total_out != nullptr, "tail chain plan: null output");
    std::vector<TailStage> st = tail_stages_of(stages, nstages);
    static const char key = 0;
    for (TailStage& t : st)
        if (!t.wgt_packed) t.wgt_packed = &key;      // (a filter is no key of the plan)
    std::vector<TailPlanStage> plan(nstages);
    tail_chain_plan(st.data(), nstages, plan.data(), lds_total_out);
    memcpy(plan_out, plan.data(), (size_t)nstages * sizeof(TailPlanStage));
    API_END
}
int ssd_op_tail_chain_bf16(const ssd_tail_stage* stages, int nstages, int b, void* stream) {
    API_BEGIN
    hipStream_t s = (hipStream_t)stream;
    std::vector<TailStage> st = tail_stages_of(stages, nstages);
    for (int i = 0; i < nstages; ++i)
        SSD_REQUIRE(st[i].wgt_packed != nullptr && st[i].src != nullptr && st[i].dst != nullptr, "tail chain: stage %d has a null tensor", i);
    {   // a list the chain refuses is refused before the pack launch reads a filter by its shape
        std::vector<TailPlanStage> plan(nstages);
        int lds_total = 0;
        tail_chain_plan(st.data(), nstages, plan.data(), &lds_total);
    }
    int device = 0;
    HIP_OK(hipGetDevice(&device));
    HipOwner tmp(device);
    TailTables tables{tmp, {}};
    std::vector<TailPackItem> items(nstages);
    size_t total = 0;      // (one image of all packed filters, back to back: the step's wq_tail_)
    for (int i = 0; i < nstages; ++i) total += tail_chain_packed_elems(st[i].d, st[i].dgrad);
    char* store = static_cast<char*>(tmp.mem(total * 2));
    for (int i = 0; i < nstages; ++i) {
        items[i] = TailPackItem{st[i].d, st[i].dgrad, st[i].wgt_packed, store};
        st[i].wgt_packed = store;
        store += tail_chain_packed_elems(st[i].d, st[i].dgrad) * 2;
    }
    tail_chain_pack_filters(items.data(), nstages, s);
    tail_chain_bf16(st.data(), nstages, b, st[0].dgrad ? "tail_dgrad_bf16" : "tail_fwd_bf16", s, tables);
    HIP_OK(hipStreamSynchronize(s));
    API_END
}
int ssd_op_conv2d_wgrad_group_bf16(const ssd_wgrad_item* items, int n, float weight_decay, int b, void* stream) {
    API_BEGIN
    SSD_REQUIRE(items != nullptr && n >= 1 && n <= 4096, "grouped weight gradient: no layer list (%d layers)", n);
    std::vector<WgradGroupItem> v(n);
    for (int i = 0; i < n; ++i) {
        const ssd_wgrad_item& a = items[i];
        v[i].d = mk(b, a.hi, a.wi, a.ci, a.ho, a.wo, a.co, a.kh, a.kw, a.stride, a.dil, a.pad_h, a.pad_w);
        v[i].x = (const bf16_t*)a.x; v[i].dy = (const bf16_t*)a.dy; v[i].dw = a.dw; v[i].dbias = a.dbias; v[i].w = a.w;
    }
    conv_wgrad_group_bf16(v.data(), n, weight_decay, (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_first_fwd_bf16(const float* x, const float* w, const float* bias, void* y, int b, int hi, int wi, int ci, int ho,
                                 int wo, int co, int kh, int kw, int stride, int dil, int pad_h, int pad_w, int relu,
                                 void* stream) {
    API_BEGIN
    conv_first_fwd_bf16(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), x, w, bias, (bf16_t*)y, relu != 0,
                        (hipStream_t)stream);
    API_END
}
size_t ssd_op_conv2d_first_wgrad_bf16_ws_floats(int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride,
                                                int dil, int pad_h, int pad_w) {
    return conv_first_wgrad_bf16_ws_floats(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w));
}
int ssd_op_conv2d_first_wgrad_bf16(const float* x, const void* dy, float* dw, float* dbias, const float* w, float weight_decay,
                                   float* ws, int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride,
                                   int dil, int pad_h, int pad_w, void* stream) {
    API_BEGIN
    conv_first_wgrad_bf16(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), x, (const bf16_t*)dy, dw, dbias, w,
                          weight_decay, ws, (hipStream_t)stream);
    API_END
}
namespace {
struct WinoWs {      // the op-level scratch: [U][Uflip][V][Mx][Yt][Ya][slabs]
    float *U, *Uf, *V, *Mx, *Yt, *Ya, *slabs;
    size_t total;
    WinoWs(const ConvDesc& d, float* ws) {
        const size_t cop = wino_kpad(d.Co), u = (size_t)36 * d.Ci * cop, t = (size_t)36 * wino_tiles(d);
        U = ws; Uf = U + u; V = Uf + u; Mx = V + t * d.Ci; Yt = Mx + t * std::max((size_t)d.Ci, cop); Ya = Yt + t * cop; slabs = Ya + t * cop;
        total = (size_t)(slabs - ws) + wino_wgrad_ws_floats(d);
    }
};
}  // namespace
size_t ssd_op_conv2d_wino_ws_floats(int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil,
                                    int pad_h, int pad_w) {
    const ConvDesc d = mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w);
    return wino_applicable(d) ? WinoWs(d, nullptr).total : 0;
}
size_t ssd_op_conv2d_wino_bits_words(int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil,
                                     int pad_h, int pad_w) {
    const ConvDesc d = mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w);
    return wino_applicable(d) ? (size_t)wino_tiles(d) * (d.Ci / 4) : 0;
}
int ssd_op_conv2d_wino_fwd(const float* x, const float* w, const float* bias, float* y, float* y_pool, void* rec, void* relu_bits, float* ws,
                           int flags, int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil,
                           int pad_h, int pad_w, int relu, void* stream) {
    API_BEGIN
    const ConvDesc d = mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w);
    SSD_REQUIRE(wino_applicable(d), "winograd: 3x3 / stride 1 / SAME layers (any dilation), Ci in multiples of 32, Co of 4");
    const WinoWs k(d, ws);
    if (!(flags & 1)) {
        HIP_OK(hipMemsetAsync(k.Uf, 0, (size_t)36 * d.Ci * wino_kpad(d.Co) * sizeof(float), (hipStream_t)stream));      // the pad rows
        wino_filter(d, w, k.U, k.Uf, (hipStream_t)stream);
    }
    wino_fwd(d, x, k.U, bias, y, relu != 0, k.V, (size_t)wino_tiles(d) * d.Ci, k.Mx, y_pool, rec, (hipStream_t)stream, relu_bits,
             (flags & 4) != 0, (flags & 8) != 0);
    API_END
}
int ssd_op_conv2d_wino_dgrad(const float* dy, const float* w, float* dx, const float* mask, const void* mask_bits, int accumulate,
                             const void* rec, int uh, int uw, float* ws, int flags, int b, int hi, int wi, int ci, int ho, int wo, int co,
                             int kh, int kw, int stride, int dil, int pad_h, int pad_w, void* stream) {
    API_BEGIN
    const ConvDesc d = mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w);
    SSD_REQUIRE(wino_applicable(d), "winograd: 3x3 / stride 1 / SAME layers (any dilation), Ci in multiples of 32, Co of 4");
    const WinoWs k(d, ws);
    if (!(flags & 1)) {
        HIP_OK(hipMemsetAsync(k.Uf, 0, (size_t)36 * d.Ci * wino_kpad(d.Co) * sizeof(float), (hipStream_t)stream));      // the pad rows
        wino_filter(d, w, k.U, k.Uf, (hipStream_t)stream);
    }
    wino_bwd_transform(d, dy, k.Yt, nullptr, (hipStream_t)stream, (flags & 8) != 0);
    wino_dgrad(d, k.Yt, k.Uf, dx, mask, accumulate != 0, k.Mx, rec, uh, uw, (hipStream_t)stream, mask_bits, (flags & 4) != 0);
    API_END
}
int ssd_op_conv2d_wino_wgrad(const float* x, const float* dy, float* dw, float* dbias, const float* w, float weight_decay, float* ws,
                             int flags, int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil,
                             int pad_h, int pad_w, void* stream) {
    API_BEGIN
    const ConvDesc d = mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w);
    SSD_REQUIRE(wino_applicable(d), "winograd: 3x3 / stride 1 / SAME layers (any dilation), Ci in multiples of 32, Co of 4");
    const WinoWs k(d, ws);
    const size_t vps = (size_t)wino_tiles(d) * d.Ci;
    if (!(flags & 2)) {      // the input's transform: through wino_fwd's first kernel would need a filter; use the dy transform's B^T form on x
        ConvDesc dx = d;
        dx.Co = d.Ci; dx.Ho = d.Hi; dx.Wo = d.Wi;
        wino_bwd_transform(dx, x, k.V, nullptr, (hipStream_t)stream, (flags & 8) != 0);
    }
    wino_bwd_transform(d, dy, nullptr, k.Ya, (hipStream_t)stream, (flags & 8) != 0);
    wino_wgrad(d, k.V, vps, k.Ya, dw, dbias, w, weight_decay, k.slabs, (hipStream_t)stream, (flags & 8) != 0);
    API_END
}
int ssd_op_wino_bwd_transform(const float* dy, float* Yt, float* Ya, int b, int h, int w, int co, int dil, int flags, void* stream) {
    API_BEGIN
    const ConvDesc d = mk(b, h, w, 32, h, w, co, 3, 3, 1, dil, dil, dil);      // (the transforms know nothing of the layer's input: any valid Ci)
    SSD_REQUIRE(wino_applicable(d), "winograd: 3x3 / stride 1 / SAME layers (any dilation), Ci in multiples of 32, Co of 4");
    SSD_REQUIRE(Yt && Ya, "ssd_op_wino_bwd_transform: both outputs are required");
    wino_bwd_transform(d, dy, Yt, Ya, (hipStream_t)stream, (flags & 8) != 0, (flags & 16) != 0);
    API_END
}
int ssd_op_wino_filter_flip_plan(const float* const* w, float* const* Uf, const int* ci, const int* co, int n, int flags, void* stream) {
    API_BEGIN
    WinoFilterPlan plan;
    for (int i = 0; i < n; ++i) plan.add(w[i], nullptr, Uf[i], ci[i], co[i]);
    wino_filter_plan(plan, false, true, (hipStream_t)stream, (flags & 1) != 0);
    API_END
}
size_t ssd_op_conv2d_wgrad_ws_floats(int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride,
                                     int dil, int pad_h, int pad_w) {
    return conv_wgrad_ws_floats(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w));
}
int ssd_op_conv2d_wgrad(const float* x, const float* dy, float* dw, float* dbias, const float* w, float weight_decay,
                        float* ws, int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil,
                        int pad_h, int pad_w, void* stream) {
    API_BEGIN
    conv_wgrad(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), x, dy, dw, dbias, w, weight_decay, ws,
               (hipStream_t)stream);
    API_END
}
// fp8 inference kernels (conv_fp8.hip)
int ssd_op_quantize_fp8(const void* x, int x_f32, size_t n, float scale, void* y8, void* stream) {
    API_BEGIN
    quantize_fp8(x, x_f32 != 0, n, scale, (unsigned char*)y8, (hipStream_t)stream);
    API_END
}
int ssd_op_absmax_bf16(const void* x, size_t n, float* out_dev, int accumulate, void* stream) {
    API_BEGIN
    absmax_bf16((const bf16_t*)x, n, out_dev, accumulate != 0, (hipStream_t)stream);
    API_END
}
int ssd_op_quantize_filter_fp8(const float* w, void* w8, float* s_w, int taps, int ci, int co, void* stream) {
    API_BEGIN
    SSD_REQUIRE(w && w8 && s_w && taps >= 1 && ci >= 1 && co >= 1, "quantize_filter_fp8: null argument or empty filter");
    FilterQuantPlan plan;
    plan.add(0, 0, 0, taps, ci, co);
    quantize_filters_fp8(plan, w, (unsigned char*)w8, s_w, (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_fwd_fp8(const void* x8, const void* w8, float s_in, const float* s_w, const float* bias, void* y, void* y8,
                          int out_mode, float s_out, int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride,
                          int dil, int pad_h, int pad_w, int relu, void* stream) {
    API_BEGIN
    conv_fwd_fp8(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), (const unsigned char*)x8, (const unsigned char*)w8, s_in,
                 s_w, bias, y, (unsigned char*)y8, out_mode, s_out, relu != 0, (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_fwd_fp8_bigk(const void* x8, const void* w8, float s_in, const float* s_w, const float* bias, void* y, void* y8,
                               int out_mode, float s_out, int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride,
                               int dil, int pad_h, int pad_w, int relu, void* stream) {
    API_BEGIN
    conv_bigk_fwd_fp8(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), (const unsigned char*)x8, (const unsigned char*)w8,
                      s_in, s_w, bias, y, (unsigned char*)y8, out_mode, s_out, relu != 0, (hipStream_t)stream);
    API_END
}
int ssd_op_maxpool_fwd_fp8(const void* x8, void* y8, int b, int hi, int wi, int c, int ho, int wo, int k, int stride, int pad_h,
                           int pad_w, void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, ho, wo, k, stride, pad_h, pad_w};
    maxpool_fwd_fp8(d, (const unsigned char*)x8, (unsigned char*)y8, (hipStream_t)stream);
    API_END
}
// mxfp8 inference kernels (conv_mxfp8.hip)
int ssd_op_quantize_mxfp8(const void* x, int x_f32, size_t rows, int c, void* y8, void* yscales, void* stream) {
    API_BEGIN
    quantize_mxfp8(x, x_f32 != 0, rows, c, (unsigned char*)y8, (unsigned char*)yscales, (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_fwd_mxfp8(const void* x8, const void* xscales, const void* w8, const float* s_w, const float* bias, void* y, void* y8,
                            void* yscales, int out_mode, int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride,
                            int dil, int pad_h, int pad_w, int relu, void* stream) {
    API_BEGIN
    conv_fwd_mxfp8(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), (const unsigned char*)x8, (const unsigned char*)xscales,
                   (const unsigned char*)w8, s_w, bias, y, (unsigned char*)y8, (unsigned char*)yscales, out_mode, relu != 0, (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_fwd_mxfp8_bigk(const void* x8, const void* xscales, const void* w8, const float* s_w, const float* bias, void* y, void* y8,
                                 void* yscales, int out_mode, int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride,
                                 int dil, int pad_h, int pad_w, int relu, void* stream) {
    API_BEGIN
    conv_bigk_fwd_mxfp8(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), (const unsigned char*)x8, (const unsigned char*)xscales,
                        (const unsigned char*)w8, s_w, bias, y, (unsigned char*)y8, (unsigned char*)yscales, out_mode, relu != 0, (hipStream_t)stream);
    API_END
}
int ssd_op_maxpool_fwd_mxfp8(const void* x8, const void* xscales, void* y8, void* yscales, int b, int hi, int wi, int c, int ho, int wo, int k,
                             int stride, int pad_h, int pad_w, void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, ho, wo, k, stride, pad_h, pad_w};
    maxpool_fwd_mxfp8(d, (const unsigned char*)x8, (const unsigned char*)xscales, (unsigned char*)y8, (unsigned char*)yscales, (hipStream_t)stream);
    API_END
}
// mxfp6 inference kernels (conv_mxfp6.hip)
int ssd_op_quantize_mxfp6(const void* x, int x_f32, size_t rows, int c, void* y6, void* yscales, void* stream) {
    API_BEGIN
    quantize_mxfp6(x, x_f32 != 0, rows, c, (unsigned char*)y6, (unsigned char*)yscales, (hipStream_t)stream);
    API_END
}
int ssd_op_quantize_filter_mxfp6(const float* w, void* w6, void* wscales, int taps, int ci, int co, void* stream) {
    API_BEGIN
    SSD_REQUIRE(w && w6 && wscales && taps >= 1 && ci >= 1 && co >= 1, "quantize_filter_mxfp6: null argument or empty filter");
    FilterQuantPlan plan;
    plan.add(0, 0, 0, taps, ci, co);
    quantize_filters_mxfp6(plan, w, (unsigned char*)w6, (unsigned char*)wscales, (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_fwd_mxfp6(const void* x6, const void* xscales, const void* w6, const void* wscales, const float* bias, void* y, void* y6,
                            void* yscales, int out_mode, int b, int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride,
                            int dil, int pad_h, int pad_w, int relu, void* stream) {
    API_BEGIN
    conv_fwd_mxfp6(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), (const unsigned char*)x6, (const unsigned char*)xscales,
                   (const unsigned char*)w6, (const unsigned char*)wscales, bias, y, (unsigned char*)y6, (unsigned char*)yscales, out_mode, relu != 0,
                   (hipStream_t)stream);
    API_END
}
int ssd_op_maxpool_fwd_mxfp6(const void* x6, const void* xscales, void* y6, void* yscales, int b, int hi, int wi, int c, int ho, int wo, int k,
                             int stride, int pad_h, int pad_w, void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, ho, wo, k, stride, pad_h, pad_w};
    maxpool_fwd_mxfp6(d, (const unsigned char*)x6, (const unsigned char*)xscales, (unsigned char*)y6, (unsigned char*)yscales, (hipStream_t)stream);
    API_END
}
int ssd_op_maxpool_fwd(const float* x, float* y, int b, int hi, int wi, int c, int ho, int wo, int k, int stride, int pad_h,
                       int pad_w, void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, ho, wo, k, stride, pad_h, pad_w};
    maxpool_fwd(d, x, y, (hipStream_t)stream);
    API_END
}
int ssd_op_maxpool_bwd(const float* x, const float* dy, float* dx, int accumulate, int relu_mask, int b, int hi, int wi, int c,
                       int ho, int wo, int k, int stride, int pad_h, int pad_w, void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, ho, wo, k, stride, pad_h, pad_w};
    DevBuf ws(maxpool_bwd_ws_bytes(d));
    maxpool_bwd(d, x, dy, dx, accumulate != 0, relu_mask != 0, maxpool_bwd_ws_bytes(d) ? ws.p : nullptr, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));     // the scratch dies here
    API_END
}
// the bf16 storage forms of the two entry points above: the same dispatch (ops.hip maxpool_fwd_t / maxpool_bwd_t) on bf16_t
int ssd_op_maxpool_fwd_bf16(const void* x, void* y, int b, int hi, int wi, int c, int ho, int wo, int k, int stride, int pad_h,
                            int pad_w, void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, ho, wo, k, stride, pad_h, pad_w};
    maxpool_fwd(d, (const bf16_t*)x, (bf16_t*)y, (hipStream_t)stream);
    API_END
}
int ssd_op_maxpool_bwd_bf16(const void* x, const void* dy, void* dx, int accumulate, int relu_mask, int b, int hi, int wi, int c,
                            int ho, int wo, int k, int stride, int pad_h, int pad_w, void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, ho, wo, k, stride, pad_h, pad_w};
    DevBuf ws(maxpool_bwd_ws_bytes(d));
    maxpool_bwd(d, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)dx, accumulate != 0, relu_mask != 0, maxpool_bwd_ws_bytes(d) ? ws.p : nullptr,
                (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));     // the scratch dies here
    API_END
}
// 3x3 stride-1 SAME pooling (mod_pool5) as the training step runs it: the forward pass writes every window's first-maximum tap
// (arg: one uint32 per window and 4 channels), the backward pass reads it (ops.h maxpool_fwd_arg / maxpool_bwd_arg)
int ssd_op_maxpool_arg_fwd(const void* x, void* y, void* arg, int bf16, int b, int hi, int wi, int c, void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, hi, wi, 3, 1, 1, 1};
    if (bf16) maxpool_fwd_arg(d, (const bf16_t*)x, (bf16_t*)y, arg, (hipStream_t)stream);
    else maxpool_fwd_arg(d, (const float*)x, (float*)y, arg, (hipStream_t)stream);
    API_END
}
int ssd_op_maxpool_arg_bwd(const void* x, const void* arg, const void* dy, void* dx, int accumulate, int relu_mask, int bf16, int b,
                           int hi, int wi, int c, void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, hi, wi, 3, 1, 1, 1};
    if (bf16)
        maxpool_bwd_arg(d, (const bf16_t*)x, arg, (const bf16_t*)dy, (bf16_t*)dx, accumulate != 0, relu_mask != 0, (hipStream_t)stream);
    else maxpool_bwd_arg(d, (const float*)x, arg, (const float*)dy, (float*)dx, accumulate != 0, relu_mask != 0, (hipStream_t)stream);
    API_END
}
// 2x2 stride-2 pooling with the forward-written record (ops.h), fp32 (bf16 = 0) or bf16 storage: the unfused form of the
// fused-pool entry points below (tests compare the two bit for bit)
int ssd_op_maxpool_rec_fwd(const void* x, void* y, void* rec, int bf16, int b, int hi, int wi, int c, void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, (hi + 1) / 2, (wi + 1) / 2, 2, 2, 0, 0};
    if (bf16) maxpool_fwd_rec(d, (const bf16_t*)x, (bf16_t*)y, rec, (hipStream_t)stream);
    else maxpool_fwd_rec(d, (const float*)x, (float*)y, rec, (hipStream_t)stream);
    API_END
}
int ssd_op_maxpool_rec_bwd(const void* rec, const void* dy, void* dx, int relu_mask, int bf16, int b, int hi, int wi, int c,
                           void* stream) {
    API_BEGIN
    PoolDesc d{b, hi, wi, c, (hi + 1) / 2, (wi + 1) / 2, 2, 2, 0, 0};
    if (bf16) maxpool_bwd_rec(d, rec, (const bf16_t*)dy, (bf16_t*)dx, relu_mask != 0, (hipStream_t)stream);
    else maxpool_bwd_rec(d, rec, (const float*)dy, (float*)dx, relu_mask != 0, (hipStream_t)stream);
    API_END
}
// conv (3x3 stride 1 SAME) + bias + relu + 2x2 stride-2 max-pool in ONE kernel: y_pool [b][(ho+1)/2][(wo+1)/2][co], rec = the
// pool's record or NULL; the convolution's own output is not written (conv.h conv_fwd_pool)
int ssd_op_conv2d_fwd_pool(const float* x, const float* w, const float* bias, float* y_pool, void* rec, int b, int hi, int wi,
                           int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h, int pad_w, void* stream) {
    API_BEGIN
    conv_fwd_pool(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), x, w, bias, y_pool, rec, (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_fwd_pool_bf16(const void* x, const void* w_oi, const float* bias, void* y_pool, void* rec, int b, int hi, int wi,
                                int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h, int pad_w,
                                void* stream) {
    API_BEGIN
    conv_fwd_pool_bf16(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), (const bf16_t*)x, (const bf16_t*)w_oi, bias,
                       (bf16_t*)y_pool, rec, (hipStream_t)stream);
    API_END
}
// data gradient of a conv whose input is a pooled tensor, routed through the pool's record into the pool's input gradient
// [b][uh][uw][ci] (relu mask of that tensor's producer from the record's sign bit); the geometry is the convolution's
int ssd_op_conv2d_dgrad_unpool(const float* dy, const float* w, float* dx_unpooled, const void* rec, int uh, int uw, int b, int hi,
                               int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h, int pad_w,
                               void* stream) {
    API_BEGIN
    conv_dgrad_unpool(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), dy, w, dx_unpooled, rec, uh, uw,
                      (hipStream_t)stream);
    API_END
}
int ssd_op_conv2d_dgrad_unpool_bf16(const void* dy, const void* w_io, void* dx_unpooled, const void* rec, int uh, int uw, int b,
                                    int hi, int wi, int ci, int ho, int wo, int co, int kh, int kw, int stride, int dil, int pad_h,
                                    int pad_w, void* stream) {
    API_BEGIN
    conv_dgrad_unpool_bf16(mk(b, hi, wi, ci, ho, wo, co, kh, kw, stride, dil, pad_h, pad_w), (const bf16_t*)dy, (const bf16_t*)w_io,
                           (bf16_t*)dx_unpooled, rec, uh, uw, (hipStream_t)stream);
    API_END
}
// data gradient of a 64 -> 64 3x3 layer (geometry b, h, w) with the weight gradient of the 3-channel 3x3 first layer below it
// fused in (conv.h conv_dgrad_first_wgrad_bf16): dw1 [3][3][3][64], dbias1 [64]; dx itself is not produced
size_t ssd_op_conv2d_dgrad_first_wgrad_bf16_ws_floats(int b, int h, int w) {
    return conv_dgrad_first_wgrad_bf16_ws_floats(mk(b, h, w, 3, h, w, 64, 3, 3, 1, 1, 1, 1));
}
int ssd_op_conv2d_dgrad_first_wgrad_bf16(const void* dy, const void* w_io, const void* mask, const float* image, float* dw1, float* dbias1,
                                         const float* w1, float weight_decay, float* ws, int b, int h, int w, void* stream) {
    API_BEGIN
    conv_dgrad_first_wgrad_bf16(mk(b, h, w, 64, h, w, 64, 3, 3, 1, 1, 1, 1), (const bf16_t*)dy, (const bf16_t*)w_io, (const bf16_t*)mask,
                                mk(b, h, w, 3, h, w, 64, 3, 3, 1, 1, 1, 1), image, dw1, dbias1, w1, weight_decay, ws, (hipStream_t)stream);
    API_END
}
// which of its 2x2 pools the handle runs fused: bit 0 of out[i] = forward (producer's epilogue), bit 1 = backward (consumer's
// data gradient); i counts the 2x2 stride-2 pools in graph order; *count = their number
int ssd_pool_fusion(ssd_handle h, int* out, int cap, int* count) {
    API_BEGIN_NET(h)
    n.pool_fusion(out, cap, count);
    API_END
}
// measurement aid (tools/step_time.py): drop groups of launches from every handle's step ("" / NULL = none); results are WRONG
int ssd_debug_set_ablate(const char* tokens) {
    API_BEGIN
    set_ablate(tokens);
    API_END
}
int ssd_grads_to_bf16(int device, const float* grads_dev, void* msg_dev, size_t count, void* stream) {
    API_BEGIN
    DeviceGuard guard(device);
    grads_to_bf16(grads_dev, msg_dev, count, (hipStream_t)stream);
    API_END
}
int ssd_grads_from_bf16(int device, const void* msg_dev, float* grads_dev, size_t count, void* stream) {
    API_BEGIN
    DeviceGuard guard(device);
    grads_from_bf16(msg_dev, grads_dev, count, (hipStream_t)stream);
    API_END
}
size_t ssd_op_grad_norm_ws_bytes(size_t n) { return grad_norm_ws_bytes(n); }
int ssd_op_momentum_update_clipped(float* w, float* acc, const float* g, size_t n, float lr, float momentum, float grad_scale,
                                   float max_norm, void* ws_dev, float* report_dev, void* stream) {
    API_BEGIN
    check_grad_clip(max_norm);
    SSD_REQUIRE(w && acc && g && (max_norm == 0.f || ws_dev), "null buffer");
    momentum_update_clipped(w, acc, g, n, lr, momentum, grad_scale, max_norm, ws_dev, report_dev, (hipStream_t)stream);
    API_END
}
int ssd_op_adamw_update(float* w, float* m, float* v, const float* g, size_t n, size_t n_decay, float lr, float beta1, float beta2,
                        float eps, float decay, long long t, float grad_scale, float max_norm, void* ws_dev, float* report_dev,
                        void* stream) {
    API_BEGIN
    adamw_check(beta1, beta2, eps, decay);
    check_grad_clip(max_norm);
    SSD_REQUIRE(w && m && v && g && (max_norm == 0.f || ws_dev), "null buffer");
    adamw_update(w, m, v, g, n, n_decay, lr, beta1, beta2, eps, decay, t, grad_scale, max_norm, ws_dev, report_dev, (hipStream_t)stream);
    API_END
}
int ssd_op_ema_update(float* e, const float* w, size_t n, float decay, long long t, void* stream) {
    API_BEGIN
    ema_check(decay);
    check_ema_step(t);
    SSD_REQUIRE(n % 4 == 0, "weight EMA: arena size must be a multiple of 4");
    SSD_REQUIRE(e && w, "null buffer");
    ema_update(e, w, n, decay, t, (hipStream_t)stream);
    API_END
}
int ssd_op_ema_swap(float* a, float* b, size_t n, void* stream) {
    API_BEGIN
    SSD_REQUIRE(n % 4 == 0, "weight EMA: arena size must be a multiple of 4");
    SSD_REQUIRE(a && b, "null buffer");
    ema_swap(a, b, n, (hipStream_t)stream);
    API_END
}
int ssd_op_clock_monitor(unsigned* out_dev, int nsamples, unsigned period_ticks, void* stream) {
    API_BEGIN
    SSD_REQUIRE(out_dev && nsamples >= 1 && period_ticks >= 100, "bad arguments");
    clock_monitor(out_dev, nsamples, period_ticks, (hipStream_t)stream);
    API_END
}
int ssd_op_l2norm_fwd(const float* x, const float* scale, float* y, int npix, int c, void* stream) {
    API_BEGIN
    l2norm_fwd(npix, c, x, scale, y, (hipStream_t)stream);
    API_END
}
size_t ssd_op_l2norm_bwd_ws_floats(int npix, int c) { return l2norm_bwd_ws_floats(npix, c); }
int ssd_op_l2norm_bwd(const float* x, const float* scale, const float* dy, float* dx, float* dscale, float* ws, int npix,
                      int c, void* stream) {
    API_BEGIN
    l2norm_bwd(npix, c, x, scale, dy, dx, dscale, ws, (hipStream_t)stream);
    API_END
}
// bf16 storage of x / y / dy / dx; scale, dscale and ws stay fp32
int ssd_op_l2norm_fwd_bf16(const void* x, const float* scale, void* y, int npix, int c, void* stream) {
    API_BEGIN
    l2norm_fwd(npix, c, (const bf16_t*)x, scale, (bf16_t*)y, (hipStream_t)stream);
    API_END
}
int ssd_op_l2norm_bwd_bf16(const void* x, const float* scale, const void* dy, void* dx, float* dscale, float* ws, int npix, int c,
                           void* stream) {
    API_BEGIN
    l2norm_bwd(npix, c, (const bf16_t*)x, scale, (const bf16_t*)dy, (bf16_t*)dx, dscale, ws, (hipStream_t)stream);
    API_END
}

// the multibox loss on a caller-given head layout: the step's own launchers (ops.h) on the caller's buffers
static HeadLayout loss_op_layout(int nmaps, const int* hw, const int* nj, int num_classes, int b, int b_off, int b_total) {
    SSD_REQUIRE(hw && nj, "null layout");
    SSD_REQUIRE(num_classes >= 1 && num_classes <= MAX_CLASSES, "num_classes must be 1..%d", MAX_CLASSES);
    SSD_REQUIRE(b >= 1 && b_off >= 0 && b_off + b <= b_total, "samples %d..%d of %d", b_off, b_off + b, b_total);
    return head_layout(nmaps, hw, nj, num_classes + 5);
}
size_t ssd_op_multibox_loss_ws_bytes(int nmaps, const int* hw, const int* nj, int b_total, size_t* offsets, int* num_anchors) {
    try {
        const HeadLayout L = loss_op_layout(nmaps, hw, nj, 1, 1, 0, b_total);      // the workspace does not depend on the class count
        if (num_anchors) *num_anchors = L.A;
        if (offsets) {
            alignas(16) static char base;          // never dereferenced: the carve is pointer arithmetic only
            LossWork w;
            loss_work_carve(w, &base, b_total, L.A);
            const void* parts[6] = {w.ce, w.sl1, w.pos, w.sel, w.sample, w.losses};
            for (int i = 0; i < 6; ++i) offsets[i] = (size_t)((uintptr_t)parts[i] - (uintptr_t)&base);
        }
        return loss_work_bytes(b_total, L.A);
    } catch (const std::exception& e) {
        ssd::set_error("%s", e.what());
        return 0;
    }
}
int ssd_op_multibox_loss(int nmaps, const int* hw, const int* nj, int num_classes, void* const* heads, const float* labels,
                         float* result, void* ws, int b, int b_off, int b_total, float bnorm, const float* filters,
                         size_t nfilters, float weight_decay, void* stream) {
    API_BEGIN
    HeadLayout L = loss_op_layout(nmaps, hw, nj, num_classes, b, b_off, b_total);
    SSD_REQUIRE(heads && labels && result && ws, "null buffer");
    for (int i = 0; i < nmaps; ++i) {
        SSD_REQUIRE(heads[i], "null head buffer %d", i);
        L.buf[i] = static_cast<float*>(heads[i]);
    }
    LossWork w;
    loss_work_carve(w, ws, b_total, L.A);
    if (filters) l2_partials(filters, nfilters, w, (hipStream_t)stream);
    multibox_loss(L, b, b_off, b_total, result, labels, w, weight_decay, bnorm, (hipStream_t)stream);
    API_END
}
int ssd_op_multibox_loss_ex(int nmaps, const int* hw, const int* nj, int num_classes, void* const* heads, const float* labels,
                            float* result, void* ws, int b, int b_off, int b_total, float bnorm, const float* filters,
                            size_t nfilters, float weight_decay, const ssd_loss_config* cfg, void* stream) {
    if (!cfg || cfg->kind == SSD_LOSS_MINING)
        return ssd_op_multibox_loss(nmaps, hw, nj, num_classes, heads, labels, result, ws, b, b_off, b_total, bnorm, filters, nfilters,
                                    weight_decay, stream);
    API_BEGIN
    check_loss_config(cfg);
    HeadLayout L = loss_op_layout(nmaps, hw, nj, num_classes, b, b_off, b_total);
    SSD_REQUIRE(heads && labels && result && ws, "null buffer");
    for (int i = 0; i < nmaps; ++i) {
        SSD_REQUIRE(heads[i], "null head buffer %d", i);
        L.buf[i] = static_cast<float*>(heads[i]);
    }
    LossWork w;
    loss_work_carve(w, ws, b_total, L.A);
    if (filters) l2_partials(filters, nfilters, w, (hipStream_t)stream);
    multibox_focal_loss(L, b, b_off, b_total, result, labels, w, weight_decay, bnorm, cfg->focal_gamma, cfg->focal_alpha,
                        (hipStream_t)stream);
    API_END
}
int ssd_op_multibox_loss_grad_ex(int nmaps, const int* hw, const int* nj, int num_classes, void* const* grads, int grads_bf16,
                                 const float* labels, const float* result, void* ws, int b, int b_off, int b_total,
                                 const ssd_loss_config* cfg, void* stream) {
    if (!cfg || cfg->kind == SSD_LOSS_MINING)
        return ssd_op_multibox_loss_grad(nmaps, hw, nj, num_classes, grads, grads_bf16, labels, result, ws, b, b_off, b_total, stream);
    API_BEGIN
    check_loss_config(cfg);
    HeadLayout L = loss_op_layout(nmaps, hw, nj, num_classes, b, b_off, b_total);
    SSD_REQUIRE(grads && labels && result && ws, "null buffer");
    for (int i = 0; i < nmaps; ++i) {
        SSD_REQUIRE(grads[i], "null gradient buffer %d", i);
        L.dbuf[i] = grads[i];
    }
    L.grad_bf16 = grads_bf16 ? 1 : 0;
    LossWork w;
    loss_work_carve(w, ws, b_total, L.A);
    multibox_focal_loss_grad(L, b, b_off, result, labels, w, cfg->focal_gamma, cfg->focal_alpha, (hipStream_t)stream);
    API_END
}
int ssd_op_multibox_loss_ex2(int nmaps, const int* hw, const int* nj, int num_classes, void* const* heads, const float* labels,
                             float* result, void* ws, int b, int b_off, int b_total, float bnorm, const float* filters,
                             size_t nfilters, float weight_decay, const ssd_loss_config* cfg, const ssd_loc_loss_config* loc,
                             void* stream) {
    if (!loc || loc->kind == SSD_LOC_SMOOTH_L1)
        return ssd_op_multibox_loss_ex(nmaps, hw, nj, num_classes, heads, labels, result, ws, b, b_off, b_total, bnorm, filters, nfilters,
                                       weight_decay, cfg, stream);
    API_BEGIN
    check_loss_config(cfg);
    check_loc_loss_config(loc);
    HeadLayout L = loss_op_layout(nmaps, hw, nj, num_classes, b, b_off, b_total);
    SSD_REQUIRE(heads && labels && result && ws, "null buffer");
    for (int i = 0; i < nmaps; ++i) {
        SSD_REQUIRE(heads[i], "null head buffer %d", i);
        L.buf[i] = static_cast<float*>(heads[i]);
    }
    LossWork w;
    loss_work_carve(w, ws, b_total, L.A);
    if (filters) l2_partials(filters, nfilters, w, (hipStream_t)stream);
    const LocLoss ll{loc->kind, loc->weight};
    if (cfg && cfg->kind == SSD_LOSS_FOCAL)
        multibox_focal_loss(L, b, b_off, b_total, result, labels, w, weight_decay, bnorm, cfg->focal_gamma, cfg->focal_alpha,
                            (hipStream_t)stream, ll);
    else
        multibox_loss(L, b, b_off, b_total, result, labels, w, weight_decay, bnorm, (hipStream_t)stream, ll);
    API_END
}
int ssd_op_multibox_loss_grad_ex2(int nmaps, const int* hw, const int* nj, int num_classes, void* const* grads, int grads_bf16,
                                  const float* labels, const float* result, void* ws, int b, int b_off, int b_total,
                                  const ssd_loss_config* cfg, const ssd_loc_loss_config* loc, void* stream) {
    if (!loc || loc->kind == SSD_LOC_SMOOTH_L1)
        return ssd_op_multibox_loss_grad_ex(nmaps, hw, nj, num_classes, grads, grads_bf16, labels, result, ws, b, b_off, b_total, cfg,
                                            stream);
    API_BEGIN
    check_loss_config(cfg);
    check_loc_loss_config(loc);
    HeadLayout L = loss_op_layout(nmaps, hw, nj, num_classes, b, b_off, b_total);
    SSD_REQUIRE(grads && labels && result && ws, "null buffer");
    for (int i = 0; i < nmaps; ++i) {
        SSD_REQUIRE(grads[i], "null gradient buffer %d", i);
        L.dbuf[i] = grads[i];
    }
    L.grad_bf16 = grads_bf16 ? 1 : 0;
    LossWork w;
    loss_work_carve(w, ws, b_total, L.A);
    const LocLoss ll{loc->kind, loc->weight};
    if (cfg && cfg->kind == SSD_LOSS_FOCAL)
        multibox_focal_loss_grad(L, b, b_off, result, labels, w, cfg->focal_gamma, cfg->focal_alpha, (hipStream_t)stream, ll);
    else
        multibox_loss_grad(L, b, b_off, result, labels, w, (hipStream_t)stream, ll);
    API_END
}
int ssd_op_multibox_loss_grad(int nmaps, const int* hw, const int* nj, int num_classes, void* const* grads, int grads_bf16,
                              const float* labels, const float* result, void* ws, int b, int b_off, int b_total, void* stream) {
    API_BEGIN
    HeadLayout L = loss_op_layout(nmaps, hw, nj, num_classes, b, b_off, b_total);
    SSD_REQUIRE(grads && labels && result && ws, "null buffer");
    for (int i = 0; i < nmaps; ++i) {
        SSD_REQUIRE(grads[i], "null gradient buffer %d", i);
        L.dbuf[i] = grads[i];
    }
    L.grad_bf16 = grads_bf16 ? 1 : 0;
    LossWork w;
    loss_work_carve(w, ws, b_total, L.A);
    multibox_loss_grad(L, b, b_off, result, labels, w, (hipStream_t)stream);
    API_END
}

}  // extern "C"
