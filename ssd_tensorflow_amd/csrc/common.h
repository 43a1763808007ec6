// Shared host-side helpers for the gfx950 SSD-VGG library.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cstdio>
#include <cstdarg>
#include <cstdint>
#include <cstring>
#include <string>
#include <stdexcept>
#include <vector>

namespace ssd {

// Thread-local last-error text returned by ssd_last_error().
void set_error(const char* fmt, ...);
const char* get_error();

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

inline void fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error(buf);
}

#define HIP_OK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) ::ssd::fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define SSD_REQUIRE(cond, ...)                         \
    do {                                               \
        if (!(cond)) ::ssd::fail(__VA_ARGS__);         \
    } while (0)

// The supported class range of every entry point (network, label encoders, decode): the decode's 64-bit candidate
// key holds the class id in bits 0-6 (boxes.hip), so 1..127 classes, i.e. at most 132 values per anchor row.
constexpr int MAX_CLASSES = 127;
inline void require_num_classes(int num_classes) {
    SSD_REQUIRE(num_classes >= 1 && num_classes <= MAX_CLASSES, "num_classes must be in 1..%d (got %d)", MAX_CLASSES, num_classes);
}

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// RAII: make `device` the calling thread's current HIP device for the scope and put the caller's
// device back afterwards.  Every handle-based or device-numbered C entry point holds one, so a rank of
// a multi-GPU job can mix calls on its own GPU with free functions without its kernels migrating.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) {
        HIP_OK(hipGetDevice(&prev));
        if (prev != device) {
            HIP_OK(hipSetDevice(device));
            switched = true;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Device memory that frees itself: an op's temporaries, and every buffer a HipOwner hands out.
struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes) { HIP_OK(hipMalloc(&p, bytes ? bytes : 16)); }
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            if (p) (void)hipFree(p);
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <typename T> T* as() { return (T*)p; }
};

// Everything a handle (or a call) takes from HIP, in one place: device memory, mapped pinned host memory, events, streams.  Its
// destructor makes `device` current, synchronises it, releases all of it and puts the caller's device back -- as a member of the
// handle it runs on destruction and when the handle's constructor throws part-way.  What a caller provides is never taken.
class HipOwner {
public:
    explicit HipOwner(int device) : device_(device) {}
    ~HipOwner() {
        int prev = device_;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device_);
        (void)hipDeviceSynchronize();
        for (hipStream_t s : streams_)
            if (s) (void)hipStreamDestroy(s);
        for (hipEvent_t e : events_)
            if (e) (void)hipEventDestroy(e);
        for (void* h : pinned_) (void)hipHostFree(h);
        mem_.clear();
        if (prev != device_) (void)hipSetDevice(prev);
    }
    HipOwner(const HipOwner&) = delete;
    HipOwner& operator=(const HipOwner&) = delete;

    // (each resource gets its slot before HIP is asked for it: a failure leaves nothing untracked)
    void* mem(size_t bytes) { return mem_.emplace_back(bytes).p; }
    void* pinned(size_t bytes, void** dev) {      // mapped: *dev = the device's view of the returned host memory
        void*& h = pinned_.emplace_back();
        HIP_OK(hipHostMalloc(&h, bytes, hipHostMallocMapped));
        HIP_OK(hipHostGetDevicePointer(dev, h, 0));
        return h;
    }
    hipEvent_t event() {
        hipEvent_t& e = events_.emplace_back();
        HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return e;
    }
    hipStream_t stream() {
        hipStream_t& s = streams_.emplace_back();
        HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return s;
    }
    // give back early what mem() / pinned() / stream() handed out; anything else (a caller's stream) is left alone
    void free_mem(void* p) {      // (hipFree waits for the device)
        auto it = std::find_if(mem_.begin(), mem_.end(), [p](const DevBuf& b) { return b.p == p; });
        if (it != mem_.end()) mem_.erase(it);
    }
    void free_pinned(void* h) {
        if (take(pinned_, h)) HIP_OK(hipHostFree(h));
    }
    void free_stream(hipStream_t s) {
        if (take(streams_, s)) (void)hipStreamDestroy(s);
    }

private:
    template <typename T> static bool take(std::vector<T>& v, T x) {
        auto it = std::find(v.begin(), v.end(), x);
        if (it == v.end()) return false;
        v.erase(it);
        return true;
    }
    int device_;
    std::vector<DevBuf> mem_;
    std::vector<void*> pinned_;
    std::vector<hipEvent_t> events_;
    std::vector<hipStream_t> streams_;
};

// Per-launch timing with HIP events on the launching stream (bench.py's roofline block).
// Off by default; a Net turns it on for its steps.  One record per kernel launch.
struct Profiler {
    struct Rec {
        std::string kernel;
        double flops, bytes;
        hipEvent_t e0, e1;
    };
    bool on = false;
    bool detailed = false;          // label records "kernel:layer"
    const char* layer = "";         // set by the executor around each op
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    hipEvent_t get();
    void reset() { recs.clear(); used = 0; }
    ~Profiler();
};
extern thread_local Profiler* g_prof;

// A launch can carry the event its consumers on OTHER streams wait for (hipExtLaunchKernelGGL's stop event: the kernel packet's
// own completion signal).  An event recorded BEHIND the kernel is a packet of its own that the stream's next kernel queues
// behind: on this chip a chain of dependent kernels pays 1.5 us per link bare, 6.8 us with "record, the other stream waits and
// runs a kernel", 3.3 us when the kernel carries the event (tools/probes/event_gap.hip, profiles/r05_s_event_gap.txt).  The
// executor arms g_stop_event right before the one call whose (single, last) launch should carry it; the gather launchers take it.
extern thread_local hipEvent_t g_stop_event;
inline hipEvent_t take_stop_event() {
    hipEvent_t e = g_stop_event;
    g_stop_event = nullptr;
    return e;
}
#define SSD_LAUNCH_STOP(kern, grid, block, lds, stream, ...) \
    hipExtLaunchKernelGGL(kern, grid, block, lds, stream, nullptr, ssd::take_stop_event(), 0, __VA_ARGS__)

// RAII: records an event before and after the launches issued inside the scope.
struct ProfScope {
    hipStream_t s;
    bool active;
    size_t idx;
    ProfScope(const char* kernel, double flops, double bytes, hipStream_t stream);
    ~ProfScope();
};

// Measurement aid (net.hip): groups of launches dropped from the step, set through ssd_debug_set_ablate only
void set_ablate(const char* tokens);
bool ablated(const char* token);

// TF SAME padding: pad_total = max((ceil(in/s)-1)*s + k_eff - in, 0); before = total/2.
inline void tf_same(int in, int k, int s, int d, int* before, int* out) {
    int keff = (k - 1) * d + 1;
    int o = (in + s - 1) / s;
    int tot = (o - 1) * s + keff - in;
    if (tot < 0) tot = 0;
    *before = tot / 2;
    *out = o;
}

}  // namespace ssd
