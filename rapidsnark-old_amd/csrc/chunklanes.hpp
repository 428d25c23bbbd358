// Rows of points through the device in chunks, on two buffer sets: what scale.hip (one scalar for all points) and
// mulvec.hip (a scalar per point) share on the host.  While chunk c is copied out of pinned memory, upload, checks,
// multiplication, synth.hip's batched normalisation and download of chunk c + 1 run on the other set's stream.  The unit
// brings what differs: what it enqueues for a chunk between the upload and the normalisation, and how it judges the words
// its checks left.
#pragma once
#include "hiputil.hpp"
#include "devmem.hpp"

namespace zkp {

constexpr uint64_t LANES = 2;

// One of the buffer sets.  A chunk's whole life runs on the lane's own stream; the host copies the chunk out when it next
// needs the lane.
template <class F>
struct Lane {
    Stream st;
    StreamUploader up;
    DevBuf<Affine<F>> aff;
    DevBuf<XYZZ<F>> xyzz;
    DevBuf<F> pref;
    DevBuf<Fr> sc;                                    // a scalar per point, for the unit that uploads them
    DevBuf<uint32_t> err;                             // the words of the unit's checks
    uint8_t *pin = nullptr;                           // cap points of results, then 16 bytes for those words
    uint64_t cap = 0, off = 0, cnt = 0;               // the chunk in flight: points [off, off + cnt) of the row
    bool busy = false;
    Lane() : up(st.s) {}
    Lane(const Lane &) = delete;
    Lane &operator=(const Lane &) = delete;
    ~Lane() {
        (void)hipStreamSynchronize(st.s);
        if (pin) (void)hipHostFree(pin);
    }
    void alloc(uint64_t cap_, bool scalars, uint32_t err_words) {
        cap = cap_;
        aff.alloc(cap);
        xyzz.alloc(cap);
        pref.alloc(cap);
        if (scalars) sc.alloc(cap);
        err.alloc(err_words);
        HIP_TRY(hipHostMalloc((void **)&pin, cap * sizeof(Affine<F>) + 16, hipHostMallocDefault));
    }
    uint32_t *words() const { return reinterpret_cast<uint32_t *>(pin + cap * sizeof(Affine<F>)); }
    static uint64_t bytes(uint64_t cap_, bool scalars) { return cap_ * (sizeof(Affine<F>) + sizeof(XYZZ<F>) + sizeof(F) + (scalars ? sizeof(Fr) : 0)) + 4096; }
};

// A unit that keeps a secret on the device for its kernels declares it BEFORE its ChunkLanes member: members are destroyed
// in reverse order, so the lanes drain their streams first and the secret is wiped after nothing reads it any more.
template <class F>
struct ChunkLanes {
    Lane<F> lane[LANES];
    uint64_t cap;
    ChunkLanes(uint64_t cap_, bool scalars, uint32_t err_words) : cap(cap_ ? cap_ : 1) {
        for (auto &l : lane) l.alloc(cap, scalars, err_words);
    }
    static uint64_t bytes(uint64_t cap_, bool scalars) { return LANES * Lane<F>::bytes(cap_, scalars); }
    // out[i] = the unit's multiple of in[i], i < n (host memory, the file's bytes).  enqueue(l), on l.st.s after chunk
    // [l.off, l.off + l.cnt) has been uploaded to l.aff: the upload of what else the kernel reads, the checks (on the chunk as
    // uploaded: the normalisation writes its results there) with their words sent to l.words(), and the kernel that leaves
    // the products in l.xyzz.  judge(l), once the lane's stream has drained: throws if the words name a bad point.
    template <class Enqueue, class Judge>
    void run(uint8_t *out, const uint8_t *in, uint64_t n, Enqueue enqueue, Judge judge) {
        auto collect = [&](Lane<F> &l) {
            if (!l.busy) return;
            l.busy = false;
            HIP_TRY(hipStreamSynchronize(l.st.s));
            judge(l);
            memcpy(out + l.off * sizeof(Affine<F>), l.pin, l.cnt * sizeof(Affine<F>));
        };
        uint64_t c = 0;
        for (uint64_t off = 0; off < n; off += cap, c++) {
            Lane<F> &l = lane[c % LANES];
            collect(l);                               // the chunk two back: the other lane's goes on meanwhile
            l.off = off;
            l.cnt = n - off < cap ? n - off : cap;
            l.up.copy(l.aff.p, in + off * sizeof(Affine<F>), l.cnt * sizeof(Affine<F>));
            enqueue(l);
            normalize(l.aff.p, l.xyzz.p, l.pref.p, l.cnt, l.st.s);
            HIP_TRY(hipMemcpyAsync(l.pin, l.aff.p, l.cnt * sizeof(Affine<F>), hipMemcpyDeviceToHost, l.st.s));
            l.busy = true;
        }
        for (uint64_t j = 0; j < LANES; j++) collect(lane[(c + j) % LANES]);   // oldest first: the lowest index is named
    }
};

}   // namespace zkp
