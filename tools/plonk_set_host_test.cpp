// csrc/plonk_set_plan.hpp built for the host alone (it includes nothing of HIP), for a run under the address and
// undefined-behaviour sanitizers (tests/test_plonk_verifier_set_host.py):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I rapidsnark-old_amd/csrc tools/plonk_set_host_test.cpp
// The plan of a key-set call (the stable order by key, the ragged publics' offsets, the groups, the segments, the fold's
// ranges and workgroups) is checked against a plain restatement of the rules, on the key_of layouts of the device tests:
// an absent key, a repeated key, runs that straddle groups and chunks, chunk 7 with group 5, group 1, a group larger
// than m, all proofs under one key, and the bound segments <= keys present + groups - 1.
#include <stdio.h>

#include <map>

#include "plonk_set_plan.hpp"

using namespace zk;

static int failures = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            failures++;                                               \
        }                                                             \
    } while (0)

static std::string refusal(const std::vector<uint32_t> &key_of, const std::vector<uint64_t> &n_public, uint64_t publics_bytes) {
    std::vector<uint64_t> at;
    try {
        ps_offsets(at, "who", key_of.data(), key_of.size(), n_public, publics_bytes);
    } catch (const std::invalid_argument &e) {
        return e.what();
    }
    return "";
}

// one call of m proofs in chunks of `chunk` and groups of `group`, against the rules restated
static void check_call(const std::vector<uint32_t> &key_of, const std::vector<uint64_t> &n_public, uint64_t chunk, uint64_t group_knob) {
    const uint64_t m = key_of.size();
    uint64_t total = 0;
    for (uint32_t k : key_of) total += n_public[k] * 32;
    std::vector<uint64_t> at;
    ps_offsets(at, "who", key_of.data(), m, n_public, total);
    CHECK(at.size() == m + 1 && at[m] == total);
    for (uint64_t i = 0, run = 0; i < m; i++) {
        CHECK(at[i] == run);
        run += n_public[key_of[i]] * 32;
    }
    const uint64_t cap = m < chunk ? m : chunk, group = group_knob < cap ? group_knob : cap;
    PlonkSetChunk c(n_public.size());
    const PlonkSetCallStats st = ps_call_stats(c, key_of.data(), at, m, cap, group);
    uint64_t groups = 0, max_group_segs = 0, max_pub = 0;
    for (uint64_t off = 0; off < m; off += cap) {
        const uint64_t cnt = m - off < cap ? m - off : cap;
        c.order(key_of.data() + off, at.data() + off, cnt);
        // the restated order: positions sorted by (key, position)
        std::vector<uint32_t> want(cnt);
        for (uint64_t i = 0; i < cnt; i++) want[i] = (uint32_t)i;
        std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return key_of[off + a] < key_of[off + b]; });
        CHECK(c.src == want && c.key.size() == cnt && c.pub_at.size() == cnt && c.cnt == cnt);
        std::map<uint32_t, uint64_t> counts;
        for (uint64_t i = 0; i < cnt; i++) {
            CHECK(c.key[i] == key_of[off + c.src[i]]);
            CHECK(c.pub_at[i] == at[off + c.src[i]] - at[off]);
            CHECK(c.pub_at[i] + n_public[c.key[i]] * 32 <= at[off + cnt] - at[off]);
            counts[c.key[i]]++;
        }
        CHECK(c.present.size() == counts.size());
        for (size_t q = 0; q < c.present.size(); q++) {
            CHECK(q == 0 || c.present[q - 1] < c.present[q]);
            CHECK(c.count[c.present[q]] == counts[c.present[q]]);
        }
        max_pub = std::max(max_pub, at[off + cnt] - at[off]);

        c.groups(group);
        const uint64_t ng = (cnt + group - 1) / group;
        CHECK(c.ngroups == ng && c.group_seg0.size() == ng + 1 && c.group_seg0[0] == 0 && c.group_seg0[ng] == c.segs.size() && c.seg_key.size() == c.segs.size());
        CHECK(c.segs.size() <= ps_seg_bound(c.present.size(), ng));
        // the segments restated: a new one wherever the key changes or a group begins
        uint64_t nseg = 0;
        for (uint64_t i = 0; i < cnt; i++) {
            if (i == 0 || i % group == 0 || c.key[i] != c.key[i - 1]) {
                CHECK(nseg < c.segs.size() && c.segs[nseg].lo == i && c.segs[nseg].key == c.key[i] && c.segs[nseg].group == i / group);
                CHECK(c.seg_key[nseg] == c.key[i]);
                if (i % group == 0) CHECK(c.group_seg0[i / group] == nseg);
                nseg++;
            }
            CHECK(c.segs[nseg - 1].hi > i);
        }
        CHECK(nseg == c.segs.size());
        for (size_t s = 0; s < c.segs.size(); s++) CHECK(c.segs[s].hi == (s + 1 < c.segs.size() ? c.segs[s + 1].lo : cnt));
        for (uint64_t g = 0; g < ng; g++) max_group_segs = std::max<uint64_t>(max_group_segs, c.group_seg0[g + 1] - c.group_seg0[g]);
        CHECK(c.max_group_segs <= max_group_segs && c.max_group_segs <= std::min<uint64_t>(group, n_public.size()));
        groups += ng;

        // the fold under the call's stride: every slot once in a segment range and once in its group's generator range, every
        // workgroup inside its range, no two sums at one place, everything inside the group's array
        const uint64_t lstride = ps_l_stride(group, st.max_group_segs);
        c.fold(lstride);
        CHECK(c.ranges.size() == c.segs.size() + ng);
        std::vector<uint32_t> seg_cover(cnt, 0), gen_cover(cnt, 0);
        std::vector<uint8_t> taken(ng * lstride, 0);
        uint64_t blk = 0;
        for (size_t r = 0; r < c.ranges.size(); r++) {
            const PsRange &x = c.ranges[r];
            CHECK(x.lo < x.hi && x.hi <= cnt && x.lo / group == (x.hi - 1) / group);
            CHECK(x.blk0 == blk && x.nblk == (x.hi - x.lo + PS_FOLD_WG - 1) / PS_FOLD_WG);
            for (uint32_t b = 0; b < x.nblk; b++) CHECK(c.blocks[blk + b].range == r && c.blocks[blk + b].b == b);
            blk += x.nblk;
            const uint64_t g = x.lo / group;
            CHECK(x.out >= g * lstride + PS_PROOF_TERMS * group && x.out + x.nterms <= (g + 1) * lstride);
            for (uint32_t t = 0; t < x.nterms; t++) CHECK(!taken[x.out + t]++);
            if (x.key == PS_GENERATOR) {
                CHECK(x.t0 == PS_KEY_TERMS && x.nterms == 1 && x.lo == g * group && x.hi == std::min(cnt, (g + 1) * group));
                CHECK(x.out == g * lstride + PS_PROOF_TERMS * group + PS_KEY_TERMS * (c.group_seg0[g + 1] - c.group_seg0[g]));
                for (uint32_t i = x.lo; i < x.hi; i++) gen_cover[i]++;
            } else {
                CHECK(x.t0 == 0 && x.nterms == PS_KEY_TERMS);
                for (uint32_t i = x.lo; i < x.hi; i++) {
                    CHECK(c.key[i] == x.key);
                    seg_cover[i]++;
                }
            }
        }
        CHECK(blk == c.blocks.size());
        for (uint64_t i = 0; i < cnt; i++) CHECK(seg_cover[i] == 1 && gen_cover[i] == 1);
        CHECK(c.segs.size() <= st.max_segs && c.ranges.size() <= st.max_ranges && c.blocks.size() <= st.max_blocks);
    }
    CHECK(st.groups == groups && st.max_group_segs == max_group_segs && st.max_pub_bytes == max_pub);
}

int main() {
    // the sets of the device tests: five entries, the fifth repeats the first key's struct
    const std::vector<uint64_t> n_public = {2, 16, 0, 2, 2};

    // ---- refusals of a call
    CHECK(refusal({0, 1, 5, 9}, n_public, 0) == "who: key_of[2] = 5, the set holds 5 keys");
    CHECK(refusal({0, 1, 2}, n_public, 18 * 32 - 32) == "who: publics_bytes: 576 expected (18 values of 32 bytes), 544 given");
    CHECK(refusal({2, 2}, n_public, 0) == "" && refusal({}, n_public, 0) == "");
    CHECK(refusal({2, 2}, n_public, 32) == "who: publics_bytes: 0 expected (0 values of 32 bytes), 32 given");

    // ---- layouts
    std::vector<uint32_t> interleaved(70);              // the device test's: key 2 (no publics) absent, 0 and 4 the same struct
    const uint32_t cycle[4] = {0, 1, 3, 4};
    for (size_t i = 0; i < interleaved.size(); i++) interleaved[i] = cycle[(i * 7 + i / 5) % 4];
    std::vector<uint32_t> one_key(70, 3), runs, big;
    for (uint32_t k : {4u, 0u, 2u, 1u}) runs.insert(runs.end(), 13, k);   // runs that straddle groups of 5 and chunks of 7
    for (uint32_t i = 0; i < 600; i++) big.push_back(i < 300 ? 0 : i < 450 ? 3 : 4);   // a segment of 300, two of 150: the fold's borders
    for (const std::vector<uint32_t> &key_of : {interleaved, one_key, runs, big, std::vector<uint32_t>{1}, std::vector<uint32_t>{2, 0}})
        for (uint64_t chunk : {(uint64_t)65536, (uint64_t)7, (uint64_t)64})
            for (uint64_t group : {(uint64_t)65536, (uint64_t)5, (uint64_t)1, (uint64_t)16, (uint64_t)600, (uint64_t)256}) check_call(key_of, n_public, chunk, group);

    // ---- particular figures
    {
        std::vector<uint64_t> at;
        uint64_t total = 0;
        for (uint32_t k : big) total += n_public[k] * 32;
        ps_offsets(at, "who", big.data(), big.size(), n_public, total);
        PlonkSetChunk c(n_public.size());
        c.order(big.data(), at.data(), big.size());
        c.groups(600);
        CHECK(c.ngroups == 1 && c.segs.size() == 3 && c.max_group_segs == 3);
        c.fold(ps_l_stride(600, 3));
        CHECK(ps_l_stride(600, 3) == 9 * 600 + 8 * 3 + 1);
        CHECK(c.ranges.size() == 4 && c.ranges[0].nblk == 2 && c.ranges[1].nblk == 1 && c.ranges[2].nblk == 1 && c.ranges[3].nblk == 3 && c.blocks.size() == 7);
        CHECK(c.ranges[3].out == 9 * 600 + 24 && c.ranges[1].out == 9 * 600 + 8);
        // chunk 7 with group 5 over the runs: chunks of 7 proofs, groups of 5 and 2
        ps_offsets(at, "who", runs.data(), runs.size(), n_public, (13 * 2 + 13 * 2 + 13 * 16) * 32);
        const PlonkSetCallStats st = ps_call_stats(c, runs.data(), at, runs.size(), 7, 5);
        CHECK(st.groups == 2 * 7 + 1 && st.max_group_segs == 2);   // 52 = 7 chunks of 7 and one of 3
        CHECK(ps_seg_bound(1, 1) == 1 && ps_seg_bound(4, 3) == 6);
    }
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("plonk_set host checks OK\n");
    return 0;
}
