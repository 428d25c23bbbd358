// Host check of what the entries share on the host without HIP.  csrc/hostutil.hpp: the strict and the lax reading of a
// number from the environment, the on/off switch, the pick of the first bad point and the 0-or-1 scalar test.
// csrc/verify_batch_host.hpp: the drawn scalars, the refusal of a zero scalar, the clamp of a report's size, and
// ChunkPlan against a plain restatement of the grouping rule on the key_of layouts the device tests use.
// tests/test_verify_set_batch_host.py builds it with the address and undefined-behaviour sanitizers and runs it.
#include <stdio.h>
#include <string.h>

#include <random>
#include <set>
#include <utility>

#include "verify_batch_host.hpp"

using namespace zk;

static int bad = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            bad++;                            \
            printf("line %d: ", __LINE__);    \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
        }                                     \
    } while (0)

// ---------------------------------------------------------------- env_number
static const char *VAR = "ZKHIP_VERIFY_GROUP_KEYS";

static void expect_number(const char *value, bool good, uint64_t want) {
    if (value) setenv(VAR, value, 1);
    else unsetenv(VAR);
    const char *shown = value ? value : "(unset)";
    try {
        const uint64_t v = env_number(VAR, 7, 2, 65536, "a number of keys from 2 to 65536");
        CHECK(good && v == want, "'%s': got %llu", shown, (unsigned long long)v);
    } catch (const std::invalid_argument &e) {
        CHECK(!good, "'%s' refused: %s", shown, e.what());
        CHECK(strcmp(e.what(), "ZKHIP_VERIFY_GROUP_KEYS: a number of keys from 2 to 65536 expected") == 0, "'%s': message '%s'", shown, e.what());
    }
}

static void test_env_number() {
    expect_number(nullptr, true, 7);
    expect_number("", true, 7);
    expect_number("2", true, 2);                      // min
    expect_number("65536", true, 65536);              // max
    expect_number("300", true, 300);
    expect_number("0", false, 0);
    expect_number("1", false, 0);                     // below min
    expect_number(" 5", false, 0);
    expect_number("+5", false, 0);
    expect_number("-5", false, 0);
    expect_number("5x", false, 0);
    expect_number("5 ", false, 0);
    expect_number("65537", false, 0);                 // max + 1
    expect_number("99999999999999999999999", false, 0);   // strtoull saturates: above max
    unsetenv(VAR);
    // the group switch as both entries read it
    unsetenv("ZKHIP_VERIFY_GROUP");
    CHECK(group_size() == 1024, "default group");
    setenv("ZKHIP_VERIFY_GROUP", "16777216", 1);
    CHECK(group_size() == (1ull << 24), "largest group");
    setenv("ZKHIP_VERIFY_GROUP", "0", 1);
    try {
        group_size();
        CHECK(false, "group 0 accepted");
    } catch (const std::invalid_argument &e) {
        CHECK(strcmp(e.what(), "ZKHIP_VERIFY_GROUP: a number of proofs from 1 to 2^24 expected") == 0, "group 0: message '%s'", e.what());
    }
    unsetenv("ZKHIP_VERIFY_GROUP");
}

// ---------------------------------------------------------------- hostutil.hpp: the two readings of a number, the switch, the pick
// What each reading took before the two became one function, worked out from that code.  Lax is the chunk_points() every
// streaming unit carried: `if (e && *e) { v = strtoull(e, &end, 10); if (*end || v < min || v > max) throw; return v; } return
// dflt;`, so what strtoull skips (blanks, a sign) passes and "-1" wraps to 2^64 - 1, above any max.  Strict is env_number as
// verify_batch_host.hpp had it: the same with `*e < '0' || *e > '9'` refused as well.
static void test_both_readings() {
    static const char *V = "ZKHIP_SCALE_CHUNK", *WHAT = "a number of points from 1 to 2^28";
    const uint64_t DFLT = 7, MAX = 1ull << 28, NO = ~0ull;       // NO: refused
    const struct {
        const char *value;
        uint64_t lax, strict;
    } rows[] = {{nullptr, DFLT, DFLT}, {"", DFLT, DFLT}, {"5", 5, 5},   {" 5", 5, NO},           {"+5", 5, NO},          {"5 ", NO, NO},
                {"-1", NO, NO},        {"0", NO, NO},    {"x", NO, NO}, {"268435456", MAX, MAX}, {"268435457", NO, NO}};
    for (const auto &r : rows)
        for (const EnvForm form : {ENV_LAX, ENV_STRICT}) {
            if (r.value) setenv(V, r.value, 1);
            else unsetenv(V);
            const uint64_t want = form == ENV_LAX ? r.lax : r.strict;
            const char *shown = r.value ? r.value : "(unset)", *mode = form == ENV_LAX ? "lax" : "strict";
            try {
                const uint64_t v = env_number(V, DFLT, 1, MAX, WHAT, form);
                CHECK(v == want, "%s '%s': got %llu", mode, shown, (unsigned long long)v);
            } catch (const std::invalid_argument &e) {
                CHECK(want == NO, "%s '%s' refused: %s", mode, shown, e.what());
                CHECK(strcmp(e.what(), "ZKHIP_SCALE_CHUNK: a number of points from 1 to 2^28 expected") == 0, "%s '%s': message '%s'", mode, shown, e.what());
            }
        }
    setenv(V, "0", 1);                                // 0 where the range holds it (the cooperative thresholds): both take it
    CHECK(env_number(V, DFLT, 0, MAX, WHAT, ENV_LAX) == 0 && env_number(V, DFLT, 0, MAX, WHAT) == 0, "0 with min 0");
    setenv(V, " 5", 1);                               // the form left out is the strict one
    try {
        env_number(V, DFLT, 1, MAX, WHAT);
        CHECK(false, "' 5' accepted by default");
    } catch (const std::invalid_argument &) {
    }
    unsetenv(V);
}

static void test_switch_and_pick() {
    static const char *V = "ZKHIP_SCALE_PLAIN";
    const struct {
        const char *value;
        bool on;
    } rows[] = {{nullptr, false}, {"", false}, {"0", false}, {"1", true}, {"00", true}};
    for (const auto &r : rows) {
        if (r.value) setenv(V, r.value, 1);
        else unsetenv(V);
        CHECK(env_switch(V) == r.on, "switch '%s'", r.value ? r.value : "(unset)");
    }
    unsetenv(V);

    const uint32_t N = NO_BAD_POINT;
    const struct {
        uint32_t h[4], kind, index;
    } picks[] = {{{N, N, N, N}, 0, N}, {{5, 5, N, N}, 1, 5}, {{N, 7, 7, N}, 2, 7}, {{N, 9, 3, N}, 3, 3}, {{N, N, N, 0}, 4, 0}};
    for (const auto &p : picks) {
        const BadPoint b = lowest_bad(p.h);
        CHECK(b.kind == p.kind && (!p.kind || b.index == p.index), "pick {%u, %u, %u, %u}: kind %u at %u", p.h[0], p.h[1], p.h[2], p.h[3], b.kind, b.index);
    }
    CHECK(strcmp(KIND_TEXT[1], "has a coordinate that is not below q") == 0 && strcmp(KIND_TEXT[2], "is not on the curve") == 0 &&
              strcmp(KIND_TEXT[3], "is not in the subgroup") == 0 && strcmp(KIND_TEXT[4], "is the point at infinity") == 0,
          "the kinds' texts");

    uint8_t s[32] = {0};
    CHECK(is_0_or_1(s), "0");
    s[0] = 1;
    CHECK(is_0_or_1(s), "1");
    s[0] = 2;
    CHECK(!is_0_or_1(s), "2");
    s[0] = 1, s[31] = 1;
    CHECK(!is_0_or_1(s), "1 + 2^248");
    s[0] = 0;
    CHECK(!is_0_or_1(s), "2^248");
}

// ---------------------------------------------------------------- scalars and the report's size
static void test_scalars() {
    const uint64_t n = 4096;
    std::vector<uint8_t> sc(n * 16);
    draw_scalars(sc.data(), n, "host test");
    std::set<std::pair<uint64_t, uint64_t>> seen;
    for (uint64_t i = 0; i < n; i++) {
        CHECK(!is_zero16(sc.data() + i * 16), "scalar %llu is zero", (unsigned long long)i);
        uint64_t w[2];
        memcpy(w, sc.data() + i * 16, 16);
        seen.insert({w[0], w[1]});
    }
    CHECK(seen.size() == n, "%zu distinct scalars of %llu", seen.size(), (unsigned long long)n);
    draw_scalars(nullptr, 0, "host test");            // nothing to draw

    uint8_t z[48];
    memset(z, 0, sizeof z);
    CHECK(is_zero16(z), "zero not seen");
    for (int b = 0; b < 16; b++) {
        z[b] = 0x80;
        CHECK(!is_zero16(z), "byte %d not seen", b);
        z[b] = 0;
    }
    z[0] = z[16 + 15] = 1;                            // scalars 0 and 1 are not zero, scalar 2 is
    refuse_zero_scalars(nullptr, 3, "entry");
    refuse_zero_scalars(z, 2, "entry");
    try {
        refuse_zero_scalars(z, 3, "entry");
        CHECK(false, "a zero scalar accepted");
    } catch (const std::invalid_argument &e) {
        CHECK(strcmp(e.what(), "entry: scalar 2 is zero") == 0, "message '%s'", e.what());
    }

    struct Report {
        uint32_t size, a;
        uint64_t b, c;
    } rep{};
    CHECK(report_size<Report>(nullptr) == 0, "no report");
    rep.size = 0;
    CHECK(report_size(&rep) == sizeof rep, "size 0");
    rep.size = 8;
    CHECK(report_size(&rep) == 8, "a shorter report");
    rep.size = sizeof rep;
    CHECK(report_size(&rep) == sizeof rep, "the whole report");
    rep.size = 4096;
    CHECK(report_size(&rep) == sizeof rep, "a longer report");
}

// ---------------------------------------------------------------- ChunkPlan
// The grouping rule restated: positions in a stable order by key; a group closes when it holds `group` positions or when
// the next position would bring a key beyond the `keys`-th into it.  Each group is a list of slots.
struct Want {
    std::vector<uint64_t> order;                      // slot -> position in the chunk
    std::vector<std::vector<uint32_t>> groups;
};
static Want restate(const uint32_t *key_of, uint64_t cnt, uint64_t group, uint64_t keys) {
    Want w;
    w.order.resize(cnt);
    for (uint64_t i = 0; i < cnt; i++) w.order[i] = i;
    std::stable_sort(w.order.begin(), w.order.end(), [&](uint64_t a, uint64_t b) { return key_of[a] < key_of[b]; });
    std::vector<uint32_t> cur;
    std::set<uint32_t> inside;
    for (uint32_t s = 0; s < cnt; s++) {
        const uint32_t k = key_of[w.order[s]];
        if (!cur.empty() && (cur.size() == group || (!inside.count(k) && inside.size() == keys))) {
            w.groups.push_back(cur);
            cur.clear();
            inside.clear();
        }
        cur.push_back(s);
        inside.insert(k);
    }
    if (!cur.empty()) w.groups.push_back(cur);
    return w;
}

struct Totals {
    uint64_t groups = 0, segs = 0;
};

// one call's chunks through one ChunkPlan object, as the entry uses it; returns the groups and segments of the call
static Totals check_plan(const char *what, const std::vector<uint32_t> &key_of, const std::vector<uint32_t> &nPublic, uint64_t group, uint64_t keys,
                         uint64_t chunk) {
    Totals t;
    ChunkPlan lay(nPublic.size());
    const uint64_t n = key_of.size();
    for (uint64_t off = 0; off < n; off += chunk) {
        const uint64_t cnt = n - off < chunk ? n - off : chunk;
        const uint32_t *ko = key_of.data() + off;
        lay.plan(ko, cnt, nPublic, group, keys);
        const Want w = restate(ko, cnt, group, keys);
        // slot order: keys rising, a key's proofs in the caller's order
        std::vector<uint64_t> filled(nPublic.size(), 0), sig_at(cnt + 1, 0);
        std::vector<uint32_t> slot_key(cnt);
        for (uint64_t i = 0; i < cnt; i++) {
            const uint64_t slot = lay.slot0[ko[i]] + filled[ko[i]]++;
            CHECK(slot < cnt && w.order[slot] == i, "%s: chunk at %llu: position %llu in slot %llu", what, (unsigned long long)off, (unsigned long long)i,
                  (unsigned long long)slot);
        }
        for (uint64_t s = 0; s < cnt; s++) {
            slot_key[s] = ko[w.order[s]];
            sig_at[s + 1] = sig_at[s] + nPublic[slot_key[s]];
        }
        CHECK(lay.npub == sig_at[cnt], "%s: %llu signals, %llu expected", what, (unsigned long long)lay.npub, (unsigned long long)sig_at[cnt]);
        for (uint32_t k : lay.present) CHECK(lay.count[k] == filled[k] && lay.pub0[k] == sig_at[lay.slot0[k]], "%s: key %u's run", what, k);
        // groups and segments
        CHECK(lay.group_seg0.size() == w.groups.size() + 1, "%s: %zu groups, %zu expected", what, lay.group_seg0.size() - 1, w.groups.size());
        if (lay.group_seg0.size() != w.groups.size() + 1) continue;
        CHECK(lay.group_seg0.back() == lay.segs.size(), "%s: the closing entry", what);
        for (size_t g = 0; g < w.groups.size(); g++) {
            const std::vector<uint32_t> &slots = w.groups[g];
            uint32_t q = lay.group_seg0[g];
            for (size_t a = 0; a < slots.size();) {   // a run of one key inside the group is a segment
                size_t b = a;
                while (b < slots.size() && slot_key[slots[b]] == slot_key[slots[a]]) b++;
                const bool have = q < lay.group_seg0[g + 1];
                CHECK(have, "%s: group %zu has too few segments", what, g);
                if (have) {
                    const Seg &sg = lay.segs[q];
                    CHECK(sg.lo == slots[a] && sg.hi == slots[b - 1] + 1 && sg.key == slot_key[slots[a]] && sg.pub_at == sig_at[slots[a]],
                          "%s: group %zu segment %u: slots %u..%u key %u", what, g, q, sg.lo, sg.hi, sg.key);
                    q++;
                }
                a = b;
            }
            CHECK(q == lay.group_seg0[g + 1], "%s: group %zu has too many segments", what, g);
            CHECK(slots.size() <= group, "%s: group %zu holds %zu", what, g, slots.size());
        }
        // the check's waves: one key each, at most 64 proofs, every slot once and in order
        uint64_t next = 0;
        for (const BWave &bw : lay.waves) {
            CHECK(bw.slot0 == next && bw.cnt >= 1 && bw.cnt <= 64 && bw.reserved == 0, "%s: wave at slot %u with %u proofs", what, bw.slot0, bw.cnt);
            if (bw.slot0 != next || (uint64_t)bw.slot0 + bw.cnt > cnt) break;
            for (uint32_t l = 0; l < bw.cnt; l++) CHECK(slot_key[bw.slot0 + l] == bw.key, "%s: wave at slot %u holds key %u", what, bw.slot0, slot_key[bw.slot0 + l]);
            CHECK(bw.pub_at == sig_at[bw.slot0], "%s: wave at slot %u: its signals", what, bw.slot0);
            // a wave ends at 64 proofs or with its key's run, so a key's run is padded nowhere
            CHECK(bw.cnt == 64 || bw.slot0 + bw.cnt == lay.slot0[bw.key] + lay.count[bw.key], "%s: wave at slot %u is short inside a run", what, bw.slot0);
            next += bw.cnt;
        }
        CHECK(next == cnt, "%s: the waves hold %llu of %llu slots", what, (unsigned long long)next, (unsigned long long)cnt);
        t.groups += w.groups.size();
        t.segs += lay.segs.size();
    }
    return t;
}

static void expect_totals(const char *what, const std::vector<uint32_t> &key_of, const std::vector<uint32_t> &nPublic, uint64_t group, uint64_t keys,
                          uint64_t chunk, uint64_t groups, uint64_t segs) {
    const Totals t = check_plan(what, key_of, nPublic, group, keys, chunk);
    CHECK(t.groups == groups && t.segs == segs, "%s (%llu, %llu): %llu groups and %llu segments, %llu and %llu expected", what, (unsigned long long)group,
          (unsigned long long)keys, (unsigned long long)t.groups, (unsigned long long)t.segs, (unsigned long long)groups, (unsigned long long)segs);
}

static void test_chunk_plan() {
    const std::vector<uint32_t> nPublic = {1, 3, 0, 2, 5};   // ragged, one key without signals
    const uint64_t whole = 65536;
    // test_a_group_closed_by_the_key_limit_and_a_chunk_that_cuts_a_run
    std::vector<uint32_t> key_of;
    for (uint32_t k = 0; k < 5; k++)
        for (int j = 0; j < 3; j++) key_of.push_back(k);
    expect_totals("three a key", key_of, nPublic, 64, 2, whole, 3, 5);     // keys {0, 1}, {2, 3}, {4}
    expect_totals("three a key", key_of, nPublic, 4, 2, whole, 4, 7);      // 0001 1122 2333 444
    key_of.clear();
    for (uint32_t i = 0; i < 120; i++) key_of.push_back(i % 2);
    expect_totals("chunks of 50", key_of, nPublic, 64, 8, 50, 3, 6);
    // test_runs_of_1_63_64_65_side_by_side_and_shuffled
    key_of.clear();
    const std::pair<uint32_t, int> runs[] = {{0, 1}, {1, 63}, {2, 64}, {4, 65}};
    for (const auto &r : runs)
        for (int j = 0; j < r.second; j++) key_of.push_back(r.first);
    std::vector<uint32_t> shuffled = key_of;
    std::mt19937_64 rng(4);
    for (size_t i = shuffled.size() - 1; i > 0; i--) std::swap(shuffled[i], shuffled[rng() % (i + 1)]);
    for (const std::vector<uint32_t> *ko : {&key_of, &shuffled}) {         // the slots are the same: the order inside a key does not show
        const char *what = ko == &key_of ? "runs side by side" : "runs shuffled";
        expect_totals(what, *ko, nPublic, 64, 8, whole, 4, 5);             // 1 + 63 | 64 | 64 | 1
        expect_totals(what, *ko, nPublic, 64, 1, whole, 5, 5);             // 1 | 63 | 64 | 64 | 1
        expect_totals(what, *ko, nPublic, 1024, 2, whole, 2, 4);           // keys {0, 1}, {2, 4}
        expect_totals(what, *ko, nPublic, 1, 1, whole, 193, 193);
    }
    // a plan object used again for a chunk with other keys forgets the chunk before
    ChunkPlan lay(5);
    const uint32_t first[] = {3, 3, 1}, second[] = {4, 0};
    lay.plan(first, 3, nPublic, 64, 8);
    lay.plan(second, 2, nPublic, 64, 8);
    CHECK(lay.present == std::vector<uint32_t>({0, 4}) && lay.count[3] == 0 && lay.count[1] == 0 && lay.segs.size() == 2 && lay.npub == 6, "a plan used twice");
}

int main() {
    test_env_number();
    test_both_readings();
    test_switch_and_pick();
    test_scalars();
    test_chunk_plan();
    if (bad) {
        printf("%d checks failed\n", bad);
        return 1;
    }
    printf("OK: env_number, scalars, report size and ChunkPlan\n");
    return 0;
}
