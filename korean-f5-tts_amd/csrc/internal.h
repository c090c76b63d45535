// Internal helpers shared by the translation units of libf5hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/f5_hip.h"

int f5_fail(int code, const char* fmt, ...);  // records the thread-local message returned by f5_last_error()
// The rules of a slice's row table (engine.hip; f5_sample_span and f5k_span_stage): rows_host[b] in [-1, prev_B), no previous row named
// twice, a previous state where a row continues, y_new where one begins.
int check_span_rows(const char* who, const int32_t* rows_host, int B, const void* prev_state, int prev_B, int prev_N, const void* y_new);
// the rules of a flow-loss span table (f5_flow_loss, f5k_flow_mix, f5k_flow_loss_reduce): 0 <= start <= end <= lens[b] (N where lens is null)
int check_flow_spans(const char* who, const int32_t* span_host, const int32_t* lens_host, int B, int N);

#define HIPCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            return f5_fail(F5_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define CHK(expr)                   \
    do {                            \
        int _r = (expr);            \
        if (_r != F5_OK) return _r; \
    } while (0)
#define KCHK() HIPCHK(hipGetLastError())

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

// What each F5_PREC_* is, stated once: the element type of its MFMA operands and typed buffers (the EngineOps<T> it runs), and what the
// engine changes around them -- split16: the backbone GEMMs as split-f16 products on f32 operands; io_split: the input / output layers
// likewise under 16-bit blocks; f8: e4m3 operands in the four block GEMMs.
enum PrecElem { PE_F32, PE_BF16, PE_F16 };
struct PrecInfo {
    bool valid;
    const char* name;
    PrecElem elem;
    bool split16, io_split, f8;
    // one of the four precisions that are an operand type by themselves: what a kernel-level entry (f5k_*) can be asked for.  f16p and f8
    // are compositions the engine makes of them.
    constexpr bool plain() const { return valid && !io_split; }
};
constexpr PrecInfo prec_info(int prec) {
    switch (prec) {
        case F5_PREC_F32: return {true, "f32", PE_F32, false, false, false};
        case F5_PREC_BF16: return {true, "bf16", PE_BF16, false, false, false};
        case F5_PREC_F16: return {true, "f16", PE_F16, false, false, false};
        case F5_PREC_F16X3: return {true, "f16x3", PE_F32, true, false, false};
        case F5_PREC_F16P: return {true, "f16p", PE_F16, false, true, false};
        case F5_PREC_F8: return {true, "f8", PE_F16, false, true, true};
    }
    return {false, "?", PE_F32, false, false, false};
}

// Bump allocator over one hipMalloc'd block; with base == nullptr it only measures (dry run).
struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
    ~Arena() {
        if (base) (void)hipFree(base);
    }
    void reset() { off = 0; }
    // The workspace rule of every stage: a call measures its plan on a dry-run Arena and reserves that many bytes here.  A block
    // that is large enough stays; growth -- a device-wide synchronisation, a free and a hipMalloc -- is the only synchronisation and
    // the only allocation of a call.  A new block is always zero-filled, so that no stage can read NaN bit patterns from padding
    // it has not written (padded K / V^T regions, GEMM K padding, dead rows).  *replaced: pointers into the old block are stale.
    int reserve(size_t need_b, bool* replaced = nullptr) {
        if (replaced) *replaced = need_b > cap;
        if (need_b <= cap) return F5_OK;
        HIPCHK(hipDeviceSynchronize());
        if (base) (void)hipFree(base);
        base = nullptr;
        cap = 0;
        HIPCHK(hipMalloc((void**)&base, need_b));
        HIPCHK(hipMemset(base, 0, need_b));
        cap = need_b;
        return F5_OK;
    }
    template <typename U> U* take(size_t n) {
        off = align_up(off, 256);
        U* p = reinterpret_cast<U*>(base + off);
        off += n * sizeof(U);
        return p;
    }
};

// Raw fp32 weights as the load entry points receive them, by state-dict name, until finalize has packed them.
struct Tensor {
    float* p = nullptr;
    std::vector<int64_t> shape;
    size_t numel() const {
        size_t n = 1;
        for (auto s : shape) n *= (size_t)s;
        return n;
    }
};

struct WeightStore {
    std::map<std::string, Tensor> t;
    ~WeightStore() { clear(); }
    void clear() {
        for (auto& kv : t)
            if (kv.second.p) (void)hipFree(kv.second.p);
        t.clear();
    }
    // device-to-device copy of one tensor, replacing an earlier one of that name (who: the calling entry point)
    int put(const char* who, const char* name, const void* dev, const int64_t* shape, int ndim, hipStream_t s) {
        if (!name || !dev || ndim < 0 || ndim > 4) return f5_fail(F5_EINVAL, "%s: bad arguments", who);
        Tensor T;
        T.shape.assign(shape, shape + ndim);
        const size_t bytes = T.numel() * sizeof(float);
        auto it = t.find(name);
        if (it != t.end()) {
            (void)hipFree(it->second.p);
            t.erase(it);
        }
        HIPCHK(hipMalloc((void**)&T.p, std::max<size_t>(bytes, 16)));
        HIPCHK(hipMemcpyAsync(T.p, dev, bytes, hipMemcpyDeviceToDevice, s));
        t[name] = T;
        return F5_OK;
    }
    const Tensor* get(const std::string& n) const {
        auto it = t.find(n);
        return it == t.end() ? nullptr : &it->second;
    }
    // the tensor of that name and exactly that shape (what: "vocos" / "bigvgan", for the message)
    int need(const std::string& n, const std::vector<int64_t>& shape, const char* what, const Tensor** out) const {
        const Tensor* x = get(n);
        if (!x) return f5_fail(F5_ESTATE, "missing %s weight '%s'", what, n.c_str());
        if (x->shape != shape) return f5_fail(F5_EINVAL, "%s weight '%s' has the wrong shape", what, n.c_str());
        *out = x;
        return F5_OK;
    }
};

// The device buffers a finalize builds (packed weights, copies of the plain ones), freed together.
struct DevPool {
    std::vector<void*> bufs;
    ~DevPool() { clear(); }
    void clear() {
        for (void* p : bufs) (void)hipFree(p);
        bufs.clear();
    }
    template <typename U> int alloc(size_t n, U** out) {
        void* p = nullptr;
        HIPCHK(hipMalloc(&p, std::max<size_t>(n * sizeof(U), 16)));
        bufs.push_back(p);
        *out = reinterpret_cast<U*>(p);
        return F5_OK;
    }
    int copy_of(const WeightStore& ws, const std::string& n, const std::vector<int64_t>& shape, const char* what, hipStream_t s,
                float** out) {
        const Tensor* x = nullptr;
        CHK(ws.need(n, shape, what, &x));
        CHK(alloc(x->numel(), out));
        HIPCHK(hipMemcpyAsync(*out, x->p, x->numel() * sizeof(float), hipMemcpyDeviceToDevice, s));
        return F5_OK;
    }
};

// scratch device buffer freed at scope exit (kernel-level test entry points only)
template <typename U> struct Scratch {
    U* p = nullptr;
    ~Scratch() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n * sizeof(U), 16)); }
};

// Host staging (pinned) for small per-call tables (time grid, lengths, segment tables): a ring of slots, each guarded by an event
// recorded after its last async copy, so that consecutive calls never synchronise the stream.
struct Staging {
    enum { NSLOT = 8 };
    char* host[NSLOT] = {};
    size_t cap[NSLOT] = {};
    hipEvent_t ev[NSLOT] = {};
    bool used[NSLOT] = {};
    int next = 0;
    ~Staging() {
        for (int i = 0; i < NSLOT; ++i) {
            if (host[i]) (void)hipHostFree(host[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
    int acquire(size_t bytes, char** out, int* slot) {
        const int i = next;
        next = (next + 1) % NSLOT;
        if (!ev[i]) HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        if (used[i]) HIPCHK(hipEventSynchronize(ev[i]));  // the copies issued from this slot NSLOT calls ago are done
        if (bytes > cap[i]) {
            if (host[i]) (void)hipHostFree(host[i]);
            host[i] = nullptr;
            cap[i] = 0;
            HIPCHK(hipHostMalloc((void**)&host[i], std::max<size_t>(bytes, 4096), hipHostMallocDefault));
            cap[i] = std::max<size_t>(bytes, 4096);
        }
        *out = host[i];
        *slot = i;
        return F5_OK;
    }
    int release(int slot, hipStream_t s) {
        HIPCHK(hipEventRecord(ev[slot], s));
        used[slot] = true;
        return F5_OK;
    }
    // one table, one copy: fill(char* host) writes `bytes` into a slot, which is held until the copy to dev_dst has run
    template <typename F> int upload(void* dev_dst, size_t bytes, hipStream_t s, F&& fill) {
        char* hb = nullptr;
        int slot = 0;
        CHK(acquire(bytes, &hb, &slot));
        fill(hb);
        HIPCHK(hipMemcpyAsync(dev_dst, hb, bytes, hipMemcpyHostToDevice, s));
        return release(slot, s);
    }
};

// The one workspace of the entry points that have no handle (silence.hip, edit.hip), per device, as long as the process lives: an
// arena for a call's device tables and scratch under the workspace rule above, the pinned ring that carries the tables down, and
// `done`, which orders a call behind the one before it when the two run on different streams (the workspace is shared); on one
// stream it is a no-op.  A call holds call_state_mutex() from the lookup to leave().
struct CallState {
    Arena arena;
    Staging stage;
    hipEvent_t done = nullptr;
    bool recorded = false;
    // the plan of a call whose workspace is its tables alone: measured, reserved, carved
    int reserve_tables(size_t bytes, char** tab) {
        CHK(arena.reserve(align_up(bytes, 256) + 256));
        arena.reset();
        *tab = arena.take<char>(bytes);
        return F5_OK;
    }
    int enter(hipStream_t s) {
        if (!done) HIPCHK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        if (recorded) HIPCHK(hipStreamWaitEvent(s, done, 0));
        return F5_OK;
    }
    int leave(hipStream_t s) {
        HIPCHK(hipEventRecord(done, s));
        recorded = true;
        return F5_OK;
    }
};
// (inline with function-local statics: one registry per program, also for a program that links a single translation unit)
inline std::mutex& call_state_mutex() {
    static std::mutex m;
    return m;
}
inline int call_state_of_current_device(CallState** out) {
    static std::map<int, CallState*> states;        // by device ordinal
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    auto it = states.find(dev);
    if (it == states.end()) it = states.emplace(dev, new CallState()).first;
    *out = it->second;
    return F5_OK;
}
