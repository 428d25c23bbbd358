// Host-side helpers of libzkhip's entry points that know nothing of the prover object: RAII around HIP memory, streams
// and the current device, the exception -> status-code boundary of the C-ABI, the admission check against the free HBM,
// the upload of a .ptau's Lagrange level and the host's root of unity.  Every translation unit with entry points includes
// it (the prover's through prover_internal.hpp), and with it hostutil.hpp, the helpers that need no HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdexcept>
#include <exception>
#include <string>
#include <thread>
#include <vector>

#include "../../include/zkhip.h"
#include "common.hpp"
#include "hipcheck.hpp"
#include "hostutil.hpp"
#include "kernels.hpp"

using namespace zk;

namespace zkp {

#define HIP_TRY(expr) ZK_HIP(expr)

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void alloc(size_t count) {
        release();
        n = count;
        if (count) HIP_TRY(hipMalloc((void **)&p, count * sizeof(T)));
    }
    void upload(const void *src, size_t count, hipStream_t s) {
        if (count) HIP_TRY(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s));
    }
    size_t bytes() const { return n * sizeof(T); }      // what alloc(n) asked for
};

// Host image -> HBM for the big zkey sections (src/binfile_utils.cpp:28-33 copies the whole file into a
// malloc'ed image first; here the image is the caller's, normally a read-only mmap of the .zkey: pageable
// and possibly not yet in the page cache).  Two pinned staging chunks: while chunk k's DMA runs, four host
// threads pull chunk k+1 out of the mapping (page faults / disk reads happen there, off the DMA's path).
// A source that is already page-locked is copied from directly.
struct StreamUploader {
    static constexpr size_t CHUNK = (size_t)64 << 20;
    uint8_t *pin[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    hipStream_t s;
    int k = 0;
    explicit StreamUploader(hipStream_t s_) : s(s_) {}
    ~StreamUploader() {
        for (int i = 0; i < 2; i++) {
            if (done[i]) {
                (void)hipEventSynchronize(done[i]);
                (void)hipEventDestroy(done[i]);
            }
            if (pin[i]) (void)hipHostFree(pin[i]);
        }
    }
    void copy(void *dst, const void *src, size_t bytes) {
        if (!bytes) return;
        hipPointerAttribute_t attr;
        const bool pinned = hipPointerGetAttributes(&attr, src) == hipSuccess && attr.type == hipMemoryTypeHost;
        (void)hipGetLastError();
        if (pinned || bytes < ((size_t)4 << 20)) {
            HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
            return;
        }
        for (size_t off = 0; off < bytes; off += CHUNK, k ^= 1) {
            const size_t len = bytes - off < CHUNK ? bytes - off : CHUNK;
            if (!pin[k]) {
                HIP_TRY(hipHostMalloc((void **)&pin[k], CHUNK, hipHostMallocDefault));
                HIP_TRY(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
            } else {
                HIP_TRY(hipEventSynchronize(done[k]));          // the DMA that last read this chunk
            }
            const uint8_t *from = (const uint8_t *)src + off;
            uint8_t *to = pin[k];
            const size_t nt = 4, per = (len / nt + 4095) & ~(size_t)4095;
            std::vector<std::thread> th;
            for (size_t t = 1; t < nt; t++) {
                const size_t lo = t * per, hi = lo + per < len ? lo + per : len;
                if (lo < hi) th.emplace_back([=] { memcpy(to + lo, from + lo, hi - lo); });
            }
            memcpy(to, from, per < len ? per : len);
            for (auto &t : th) t.join();
            HIP_TRY(hipMemcpyAsync((uint8_t *)dst + off, to, len, hipMemcpyHostToDevice, s));
            HIP_TRY(hipEventRecord(done[k], s));
        }
    }
};

// d <- level p (2^p points of pt_bytes each, from point 2^p - 1 on) of a Lagrange section of a prepared .ptau
inline void upload_level(DevBuf<uint8_t> &d, const void *section, uint32_t p, uint64_t pt_bytes, hipStream_t s) {
    const uint64_t count = 1ull << p;
    d.alloc(count * pt_bytes);
    StreamUploader up(s);
    up.copy(d.p, static_cast<const uint8_t *>(section) + (count - 1) * pt_bytes, count * pt_bytes);
}

// a non-blocking stream of an entry point's own, drained and destroyed when the call leaves
struct Stream {
    hipStream_t s = nullptr;
    Stream() { HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
};

// Scalar-vector sort workspace (one per scalar set: witness, h)
struct SortBufs {
    MsmPlan plan;
    uint64_t n = 0;
    DevBuf<uint16_t> lo;
    DevBuf<uint32_t> counts, starts, offsets, entries, codes, val, bin_counts, bin_starts;
    uint32_t total_buckets() const { return plan.sets * plan.nbuckets; }
    uint64_t max_entries() const { return (n ? n : 1) * plan.W; }
    // batch > 1: `batch` scalar vectors of n_ scalars each, sorted together into one bucket set per vector
    // precomp: 0 = tables as in the zkey, 1 = a table row per window, 2 = a row per second window (MsmPlan::precomp)
    // the plan and the size rules alone: nothing is allocated and no device is touched (zk_msm_sort's plan-only call)
    void set_plan(uint64_t n_, uint32_t window_bits, uint32_t precomp = 0, uint32_t batch = 1) {
        plan = make_msm_plan(n_ ? n_ : 1, window_bits, precomp, batch);
        n = n_ * (batch > 1 ? batch : 1);
        // sort entries are 32-bit (bit 31 = digit sign): positions n*W and, with window-precomputed
        // tables, table rows j*n + i must stay below 2^32 / 2^31
        if ((n ? n : 1) * plan.W >= (1ull << 32)) throw std::invalid_argument("MSM too large: n * windows >= 2^32 sort entries");
        if ((n ? n : 1) * msm_table_rows(plan) >= (1ull << 31)) throw std::invalid_argument("MSM too large: table rows >= 2^31");
    }
    void alloc(uint64_t n_, uint32_t window_bits, uint32_t precomp = 0, uint32_t batch = 1) {
        set_plan(n_, window_bits, precomp, batch);
        MsmSortSizes z = msm_sort_sizes(n, plan);
        lo.alloc(z.lo_u16);
        counts.alloc(z.counts_u32);
        starts.alloc(z.starts_u32);
        offsets.alloc(z.offsets_u32);
        entries.alloc(z.entries_u32);
        codes.alloc(z.codes_u32);
        val.alloc(z.val_u32);
        bin_counts.alloc(z.bin_counts_u32);
        bin_starts.alloc(z.bin_starts_u32);
    }
    void release() {
        lo.release(); counts.release(); starts.release(); offsets.release(); entries.release();
        codes.release(); val.release(); bin_counts.release(); bin_starts.release();
        n = 0; ran = false;
    }
    size_t bytes() const {
        return lo.bytes() + counts.bytes() + starts.bytes() + offsets.bytes() + entries.bytes() + codes.bytes() + val.bytes()
             + bin_counts.bytes() + bin_starts.bytes();
    }
    bool ran = false;
    void run(const Fr *scalars, hipStream_t s) {
        // ZKHIP_PROBE_SKIP_SORT=1 (-DZK_PROBES builds only; wrong sums): the sort runs once per buffer set and its result is reused —
        // what a proof costs if digits + counting sort were free (profiles/NEGATIVE_RESULTS.md item 22)
        static const bool skip = probe_env("ZKHIP_PROBE_SKIP_SORT") != nullptr;
        if (skip && ran) return;
        ran = true;
        MsmSortBufs b{offsets.p, entries.p, counts.p, starts.p, codes.p, val.p, bin_counts.p, bin_starts.p, lo.p};
        launch_msm_sort(b, scalars, n, plan, s);
    }
};

inline void need_device_count() {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) throw std::runtime_error("no HIP device available (libzkhip has no CPU fallback)");
}

// the `device` argument of an entry point: -1 (any negative value) is the calling thread's current device
inline int resolve_device(int32_t device) {
    need_device_count();
    int dev = device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    return dev;
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        HIP_TRY(hipSetDevice(dev));
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// `need` bytes must fit the current device's free HBM BEFORE anything is allocated, so that running out of memory is one
// clean error of `who` (status 2, "out of memory" in the message: host/groth16.hpp's fallback chain looks for the words)
// and never a half-made object.  The margin covers the allocator's rounding and the queues of new streams.
inline void need_hbm(const char *who, uint64_t need) {
    size_t fr = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fr, &tot));
    const uint64_t margin = need / 32 + ((uint64_t)256 << 20);
    if (fr < need + margin)
        throw HipError(std::string(who) + ": out of memory (needs " + std::to_string((need + margin) >> 20) + " MiB of HBM, " +
                       std::to_string(fr >> 20) + " MiB free)");
}

template <class Fn>
int guarded(Fn fn) {
    try {
        fn();
        return 0;
    } catch (const HipError &e) {
        set_error(std::string("HIP failure: ") + e.what());
        return 2;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

// a *_destroy entry: the object's memory is freed on its own device (obj->device), the caller's current device comes back
template <class T>
void destroy_on_device(T *obj) {
    if (!obj) return;
    int prev = -1;
    const bool switched = hipGetDevice(&prev) == hipSuccess && hipSetDevice(obj->device) == hipSuccess;
    delete obj;
    if (switched) (void)hipSetDevice(prev);
}

// a *_info entry: fill(q) sets every field but `size` of a zeroed plan, and the caller gets as much of it as plan->size says
// it has room for (an older caller's shorter struct is served)
template <class Plan, class Fill>
void info_into(const char *who, Plan *plan, Fill fill) {
    if (plan->size < 4) throw std::invalid_argument(std::string(who) + ": plan->size is not set");
    Plan q{};
    fill(q);
    q.size = plan->size < sizeof q ? plan->size : (uint32_t)sizeof q;
    memcpy(plan, &q, q.size);
}

inline uint32_t ilog2_exact(uint64_t n) {
    uint32_t l = 0;
    while ((1ull << l) < n) l++;
    if ((1ull << l) != n) throw std::invalid_argument("domainSize is not a power of two");
    return l;
}

inline uint32_t nblocks(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// XYZZ -> affine of n points by synth.hip's batched inversion, G1 or G2 by the argument types
inline void normalize(G1Affine *out, const G1XYZZ *tmp, Fq *pref, uint64_t n, hipStream_t s) { launch_normalize_g1(out, tmp, pref, n, s); }
inline void normalize(G2Affine *out, const G2XYZZ *tmp, Fq2 *pref, uint64_t n, hipStream_t s) { launch_normalize_g2(out, tmp, pref, n, s); }

}   // namespace zkp
using namespace zkp;
