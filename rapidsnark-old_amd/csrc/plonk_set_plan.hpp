// The host plan of a PLONK key-set verifier's call (include/zkhip.h, zk_plonk_verifier_set_*), in
// plain C++ with nothing of HIP, so that tools/plonk_set_host_test.cpp checks it as a stand-alone program:
//   the checks of key_of and of the ragged publics, with the byte offset of every proof's publics;
//   a chunk's stable order by key (keys rising, a key's proofs in the caller's order) as an index array, slot -> position;
//   the groups of a chunk (consecutive slots) and their segments (the proofs of one key inside one group);
//   what the segmented fold sums: a range of slots a segment (the eight key terms) and one a group (the generator's term),
//   cut into workgroups of 256 slots, and where each sum goes in the group's array of scalars.
// A group's L array is 9 group proof-point slots, then 8 bases a segment, then the generator, then (0, 0) points with zero
// scalars up to the stride, which is that of the call's largest group: both bucket multiplications keep ONE size a call.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace zk {

constexpr uint32_t PS_FOLD_WG = 256;                  // slots a workgroup of the fold's first pass
constexpr uint32_t PS_KEY_TERMS = 8, PS_PROOF_TERMS = 9, PS_GENERATOR = 0xFFFFFFFFu;

// at[i]: where proof i's publics begin, in bytes from the call's first; at[m]: the total, which publics_bytes must be
inline void ps_offsets(std::vector<uint64_t> &at, const char *who, const uint32_t *key_of, uint64_t m, const std::vector<uint64_t> &n_public,
                       uint64_t publics_bytes) {
    at.resize(m + 1);
    uint64_t total = 0;
    for (uint64_t i = 0; i < m; i++) {
        if (key_of[i] >= n_public.size())
            throw std::invalid_argument(std::string(who) + ": key_of[" + std::to_string(i) + "] = " + std::to_string(key_of[i]) + ", the set holds " +
                                        std::to_string(n_public.size()) + " keys");
        at[i] = total * 32;
        total += n_public[key_of[i]];
    }
    at[m] = total * 32;
    if (publics_bytes != total * 32)
        throw std::invalid_argument(std::string(who) + ": publics_bytes: " + std::to_string(total * 32) + " expected (" + std::to_string(total) +
                                    " values of 32 bytes), " + std::to_string(publics_bytes) + " given");
}

// the segments of a chunk are at most (keys present) + (groups) - 1: every segment but a group's first begins a key's run
inline uint64_t ps_seg_bound(uint64_t keys_present, uint64_t groups) { return keys_present + groups - 1; }
inline uint64_t ps_l_stride(uint64_t group, uint64_t max_group_segs) { return PS_PROOF_TERMS * group + PS_KEY_TERMS * max_group_segs + 1; }

struct PsSeg {
    uint32_t lo, hi, key, group;                      // slots [lo, hi) of the chunk, all of `key`, inside `group`
};
// what one sum of the fold covers: slots [lo, hi), terms t0 .. t0 + nterms - 1, in workgroups blk0 .. blk0 + nblk - 1 of the
// first pass; the sums go to scalars out .. out + nterms - 1 of the chunk's L array, where the bases stand too
struct PsRange {
    uint32_t lo, hi, blk0, nblk;
    uint32_t out, key, t0, nterms;                    // key: the segment's, PS_GENERATOR for a group's generator range
};
struct PsBlock {
    uint32_t range, b;                                // workgroup b of its range: slots lo + 256 b ..
};
static_assert(sizeof(PsRange) == 32 && sizeof(PsBlock) == 8 && sizeof(PsSeg) == 16, "layout");

struct PlonkSetChunk {
    std::vector<uint64_t> count;                      // per key: its proofs in the chunk (zero between calls of order())
    std::vector<uint32_t> present;                    // the keys with proofs in the chunk, rising
    std::vector<uint32_t> src, key;                   // per slot: the proof's position in the chunk, its key
    std::vector<uint64_t> pub_at;                     // per slot: where its publics begin, in bytes from the chunk's first
    uint64_t cnt = 0;
    // the groups (after groups())
    uint64_t group = 0, ngroups = 0, max_group_segs = 0;
    std::vector<PsSeg> segs;
    std::vector<uint32_t> group_seg0;                 // per group its first segment; one more entry closes the last
    std::vector<uint32_t> seg_key;                    // segs[].key alone, what the gather reads
    std::vector<PsRange> ranges;
    std::vector<PsBlock> blocks;
    explicit PlonkSetChunk(size_t n_keys) : count(n_keys, 0) {}

    // the proofs at positions 0 .. cnt - 1 of the chunk; at: the call's offsets of those positions (at[cnt] closes them)
    void order(const uint32_t *key_of, const uint64_t *at, uint64_t cnt_) {
        for (uint32_t k : present) count[k] = 0;
        present.clear();
        cnt = cnt_;
        for (uint64_t i = 0; i < cnt; i++)
            if (count[key_of[i]]++ == 0) present.push_back(key_of[i]);
        std::sort(present.begin(), present.end());
        std::vector<uint64_t> next(present.size());
        uint64_t slot = 0;
        for (size_t q = 0; q < present.size(); q++) {
            next[q] = slot;
            slot += count[present[q]];
            count[present[q]] = q;                    // the key's rank while the slots are dealt
        }
        src.resize(cnt), key.resize(cnt), pub_at.resize(cnt);
        for (uint64_t i = 0; i < cnt; i++) {
            const uint64_t to = next[count[key_of[i]]]++;
            src[to] = (uint32_t)i;
            key[to] = key_of[i];
            pub_at[to] = at[i] - at[0];
        }
        slot = 0;
        for (size_t q = 0; q < present.size(); q++) {  // the counts again
            count[present[q]] = next[q] - slot;
            slot = next[q];
        }
    }

    // groups of `group_` consecutive slots, the last maybe short, and their segments; no range or block yet
    void groups(uint64_t group_) {
        group = group_;
        ngroups = (cnt + group - 1) / group;
        segs.clear(), group_seg0.clear(), seg_key.clear();
        max_group_segs = 0;
        for (uint64_t g = 0; g < ngroups; g++) {
            group_seg0.push_back((uint32_t)segs.size());
            const uint64_t end = std::min(cnt, (g + 1) * group);
            for (uint64_t lo = g * group; lo < end;) {
                uint64_t hi = lo + 1;
                while (hi < end && key[hi] == key[lo]) hi++;
                segs.push_back(PsSeg{(uint32_t)lo, (uint32_t)hi, key[lo], (uint32_t)g});
                seg_key.push_back(key[lo]);
                lo = hi;
            }
            max_group_segs = std::max<uint64_t>(max_group_segs, segs.size() - group_seg0[g]);
        }
        group_seg0.push_back((uint32_t)segs.size());
    }

    // the fold's ranges and workgroups for group arrays `l_stride` apart (ps_l_stride of the CALL's largest group)
    void fold(uint64_t l_stride) {
        ranges.clear(), blocks.clear();
        auto put = [&](uint32_t lo, uint32_t hi, uint64_t out, uint32_t k, uint32_t t0, uint32_t nterms) {
            const uint32_t nblk = (hi - lo + PS_FOLD_WG - 1) / PS_FOLD_WG;
            for (uint32_t b = 0; b < nblk; b++) blocks.push_back(PsBlock{(uint32_t)ranges.size(), b});
            ranges.push_back(PsRange{lo, hi, (uint32_t)(blocks.size() - nblk), nblk, (uint32_t)out, k, t0, nterms});
        };
        for (uint64_t g = 0; g < ngroups; g++) {
            const uint64_t base = g * l_stride + PS_PROOF_TERMS * group;
            const uint32_t s0 = group_seg0[g], s1 = group_seg0[g + 1];
            for (uint32_t s = s0; s < s1; s++) put(segs[s].lo, segs[s].hi, base + PS_KEY_TERMS * (s - s0), segs[s].key, 0, PS_KEY_TERMS);
            put((uint32_t)(g * group), (uint32_t)std::min(cnt, (g + 1) * group), base + PS_KEY_TERMS * (s1 - s0), PS_GENERATOR, PS_KEY_TERMS, 1);
        }
    }
};

// what a whole call needs before its first chunk: the largest group's segments, the most segments, ranges and workgroups of a
// chunk, and the most bytes of publics of a chunk
struct PlonkSetCallStats {
    uint64_t max_group_segs = 0, max_segs = 0, max_ranges = 0, max_blocks = 0, max_pub_bytes = 0, groups = 0;
};
inline PlonkSetCallStats ps_call_stats(PlonkSetChunk &c, const uint32_t *key_of, const std::vector<uint64_t> &at, uint64_t m, uint64_t cap, uint64_t group) {
    PlonkSetCallStats st;
    for (uint64_t off = 0; off < m; off += cap) {
        const uint64_t cnt = std::min(cap, m - off);
        c.order(key_of + off, at.data() + off, cnt);
        st.max_pub_bytes = std::max(st.max_pub_bytes, at[off + cnt] - at[off]);
        if (!group) continue;
        c.groups(group);
        c.fold(ps_l_stride(group, c.max_group_segs));
        st.max_group_segs = std::max(st.max_group_segs, c.max_group_segs);
        st.max_segs = std::max<uint64_t>(st.max_segs, c.segs.size());
        st.max_ranges = std::max<uint64_t>(st.max_ranges, c.ranges.size());
        st.max_blocks = std::max<uint64_t>(st.max_blocks, c.blocks.size());
        st.groups += c.ngroups;
    }
    return st;
}

}   // namespace zk
