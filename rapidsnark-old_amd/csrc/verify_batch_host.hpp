// The host side that the batch-verification entries (and kzg.hip's batch) share and that needs no HIP: the group switch
// (hostutil.hpp's strict env_number, as the cooperative thresholds in pairing_coop.hpp), the scalars (drawn, or the
// caller's, refused when zero), the clamp of a caller's report size, and the layout of one chunk of a key set's batch.
// tools/verify_batch_host_test.cpp builds it for the host alone.
#pragma once
#include <errno.h>
#include <sys/random.h>

#include <algorithm>
#include <vector>

#include "hostutil.hpp"

namespace zk {

constexpr uint64_t DEFAULT_GROUP = 1024;              // profiles/verify_batch_timing.txt
// ZKHIP_VERIFY_GROUP: the proofs of a group, read at every call
inline uint64_t group_size() { return env_number("ZKHIP_VERIFY_GROUP", DEFAULT_GROUP, 1, 1ull << 24, "a number of proofs from 1 to 2^24"); }

inline bool is_zero16(const uint8_t *p) {
    uint8_t o = 0;
    for (int i = 0; i < 16; i++) o |= p[i];
    return o == 0;
}

// n scalars of 16 bytes from the system's random source, none zero; entry: the caller's name for the message
inline void draw_scalars(uint8_t *out, uint64_t n, const char *entry) {
    for (size_t got = 0, want = (size_t)n * 16; got < want;) {
        const ssize_t k = getrandom(out + got, want - got, 0);
        if (k < 0) {
            if (errno == EINTR) continue;
            throw std::runtime_error(std::string(entry) + ": the random source failed");
        }
        got += (size_t)k;
    }
    for (uint64_t i = 0; i < n; i++)
        while (is_zero16(out + i * 16)) {
            const ssize_t k = getrandom(out + i * 16, 16, 0);
            if (k < 0 && errno != EINTR) throw std::runtime_error(std::string(entry) + ": the random source failed");
        }
}

// a caller's scalars (null: none given): a zero one is an error of the call
inline void refuse_zero_scalars(const uint8_t *scalars16, uint64_t n, const char *entry) {
    if (!scalars16) return;
    for (uint64_t i = 0; i < n; i++)
        if (is_zero16(scalars16 + i * 16)) throw std::invalid_argument(std::string(entry) + ": scalar " + std::to_string(i) + " is zero");
}

// how many bytes of the report go back: the caller's `size` when it is set and smaller than the struct; null: none
template <class Report>
inline uint32_t report_size(const Report *report) {
    if (!report) return 0;
    return report->size && report->size < sizeof *report ? report->size : (uint32_t)sizeof *report;
}

// ---------------------------------------------------------------- a chunk of zk_vkey_set_verify_batch
struct BWave {                                        // a wave of the check: `cnt` proofs of key `key` from slot `slot0` on
    uint64_t pub_at;                                  // where the first lane's signals begin, in signals from the chunk's first
    uint32_t key, slot0, cnt, reserved;
};
static_assert(sizeof(BWave) == 24, "layout");

// The layout of one chunk: the proofs of caller positions off .. off + cnt - 1 in slots ordered by key (keys rising, a
// key's proofs in the caller's order), the waves of the check, and the groups and segments by position.
struct Seg {
    uint32_t lo, hi, key;
    uint64_t pub_at;                                  // where the signals of slot `lo` begin
};
struct ChunkPlan {
    std::vector<uint64_t> count, slot0, pub0;         // per key: its proofs in the chunk, its first slot, its first signal
    std::vector<uint32_t> present;                    // the keys with proofs in the chunk
    std::vector<BWave> waves;
    std::vector<Seg> segs;
    std::vector<uint32_t> group_seg0;                 // per group its first segment; one more entry closes the last
    uint64_t npub = 0;
    explicit ChunkPlan(size_t n_keys) : count(n_keys, 0), slot0(n_keys), pub0(n_keys) {}
    void plan(const uint32_t *key_of, uint64_t cnt, const std::vector<uint32_t> &nPublic, uint64_t group, uint64_t group_keys) {
        for (uint32_t k : present) count[k] = 0;
        present.clear();
        waves.clear();
        segs.clear();
        group_seg0.clear();
        npub = 0;
        for (uint64_t i = 0; i < cnt; i++)
            if (count[key_of[i]]++ == 0) present.push_back(key_of[i]);
        std::sort(present.begin(), present.end());
        uint64_t slot = 0, in_group = 0, keys_in_group = 0;
        for (uint32_t k : present) {
            slot0[k] = slot;
            pub0[k] = npub;
            const uint64_t end = slot + count[k];
            for (uint64_t done = 0; done < count[k]; done += 64) {
                const uint32_t live = (uint32_t)(count[k] - done < 64 ? count[k] - done : 64);
                waves.push_back(BWave{npub + done * nPublic[k], k, (uint32_t)(slot + done), live, 0});
            }
            bool fresh = true;                        // k is not yet in the open group
            while (slot < end) {
                if (in_group == 0 || (fresh && keys_in_group == group_keys)) {   // a new group opens
                    group_seg0.push_back((uint32_t)segs.size());
                    in_group = keys_in_group = 0;
                    fresh = true;
                }
                const uint64_t take = std::min(end - slot, group - in_group);
                segs.push_back(Seg{(uint32_t)slot, (uint32_t)(slot + take), k, npub + (slot - slot0[k]) * nPublic[k]});
                keys_in_group += fresh;
                fresh = false;
                in_group += take;
                slot += take;
                if (in_group == group) in_group = 0;  // full: the next proof opens a group
            }
            npub += count[k] * nPublic[k];
        }
        group_seg0.push_back((uint32_t)segs.size());
    }
};

}   // namespace zk
