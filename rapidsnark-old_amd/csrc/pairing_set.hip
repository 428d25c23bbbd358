// Verification of a mixed batch: proofs under many keys in one call (zk_vkey_set_*, include/zkhip.h).
// A set borrows existing zk_vkey objects of one device and keeps a device array with one record per key: the addresses of
// the key's IC, of its line tables of gamma and delta, of its Miller value of (alpha, beta), and its nPublic.  The kernels
// here are the counterparts of pairing.hip's and pairing_coop.hip's with one difference: the key comes from that array,
// not from the launch arguments, so a call launches the same kernels whatever the number of keys and however the proofs
// are spread over them.  What a lane or a workgroup computes is verify_lanes.hpp's and pairing_coop_dev.hpp's, the code
// the single-key kernels run: a proof gets the verdict zk_vkey_verify gives it under its key.
//
//   Up to ZKHIP_VERIFY_COOP_MAX proofs: k_set_coop, a workgroup per proof in the caller's order; workgroup i reads
//   key_of[i] and at[i], where its public signals begin.  One launch.
//   Above: a lane per proof in chunks of ZKHIP_VERIFY_CHUNK.  The host groups a chunk's proofs by key (a stable counting
//   sort over key_of, done while it copies them into staging) and pads every key's run to whole waves, so a wave has one
//   key: it reads gamma's and delta's lines with a wave-uniform address, as k_verify_miller does, and the signals of its
//   lanes lie one after another.  k_set_check, k_set_miller and k_set_final take one record per wave (key, live lanes,
//   where the wave's signals begin); the idle lanes of a run's last wave return at once.  The verdicts come back by slot
//   and are scattered to the caller's positions.  Three launches a chunk.
//
// The keys' device data never changes after zk_vkey_create, so a call takes the set's mutex alone and touches no key's
// plan, stream or buffers.
#include <algorithm>
#include <memory>
#include <mutex>

#include "hiputil.hpp"
#include "verify_lanes.hpp"
#include "pairing_coop_dev.hpp"
#include "pairing_set_internal.hpp"

namespace {

struct WaveRec {                                      // a wave of the lane path: `cnt` proofs of key `key` in its first lanes
    uint64_t pub_at;                                  // where the first lane's signals begin, in signals from the chunk's first
    uint32_t key, cnt;
};
static_assert(sizeof(WaveRec) == 16, "layout");

// ---------------------------------------------------------------- a lane per proof, a wave per run of one key
// Slot i = 64 blockIdx.x + threadIdx.x of the staged chunk.  The grid is the chunk's waves exactly; w and key are the same
// in every lane of the wave.
__global__ __launch_bounds__(64) void k_set_check(uint32_t *status, G1Affine *vkx, const uint8_t *__restrict__ proofs, const Fr *__restrict__ publics,
                                                  const WaveRec *__restrict__ waves, const KeyRec *__restrict__ keys, Fq b1, Fq2 b2) {
    const WaveRec w = waves[blockIdx.x];
    if (threadIdx.x >= w.cnt) return;
    const KeyRec key = keys[w.key];
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    verify_check_lane(status + i, vkx + i, proofs + i * 256, publics + w.pub_at + (uint64_t)threadIdx.x * key.nPublic, key.nPublic, key.ic, b1, b2);
}

__global__ __launch_bounds__(64) void k_set_miller(Fq12 *f_out, const uint32_t *__restrict__ status, const uint8_t *__restrict__ proofs,
                                                   const G1Affine *__restrict__ vkx, const WaveRec *__restrict__ waves, const KeyRec *__restrict__ keys,
                                                   const PairConsts *k) {
    const WaveRec w = waves[blockIdx.x];
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (threadIdx.x >= w.cnt || status[i] != ST_OK) return;
    const KeyRec key = keys[w.key];
    verify_miller_lane(f_out + i, proofs + i * 256, vkx + i, key.tab, key.ml_ab, k);
}

__global__ __launch_bounds__(64) void k_set_final(uint8_t *verdict, const Fq12 *f, const uint32_t *__restrict__ status, const WaveRec *__restrict__ waves,
                                                  const PairConsts *k) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (threadIdx.x >= waves[blockIdx.x].cnt) return;
    verify_final_lane(verdict + i, f + i, status[i], k);
}

// ---------------------------------------------------------------- a workgroup per proof
// at[i]: where proof i's signals begin, in signals from the call's first
__global__ __launch_bounds__(VERIFY_THREADS) void k_set_coop(uint8_t *verdict, const uint8_t *__restrict__ proofs, const Fr *__restrict__ publics,
                                                             const uint32_t *__restrict__ key_of, const uint64_t *__restrict__ at,
                                                             const KeyRec *__restrict__ keys, const PairConsts *__restrict__ k, Line *lines, Fq b1, Fq2 b2,
                                                             Fq beta) {
    const uint64_t i = blockIdx.x;
    const KeyRec key = keys[key_of[i]];
    verify_coop_proof(verdict + i, proofs + i * 256, publics + at[i], key.nPublic, key.ic, key.tab, key.ml_ab, k, lines + i * MILLER_LINES, b1, b2, beta);
}

}   // namespace

// ---------------------------------------------------------------- host
namespace {

zk_vkey_set *set_create(zk_vkey *const *keys, uint32_t n_keys) {
    if (!keys) throw std::invalid_argument("null argument");
    if (!n_keys) throw std::invalid_argument("zk_vkey_set_create: a set needs at least one key");
    for (uint32_t j = 0; j < n_keys; j++) {
        if (!keys[j]) throw std::invalid_argument("zk_vkey_set_create: key " + std::to_string(j) + " is null");
        if (keys[j]->device != keys[0]->device)
            throw std::invalid_argument("zk_vkey_set_create: key " + std::to_string(j) + " is on device " + std::to_string(keys[j]->device) + ", key 0 on device " +
                                        std::to_string(keys[0]->device) + "; a set's keys are on one device");
    }
    std::unique_ptr<zk_vkey_set> set(new zk_vkey_set);
    set->device = keys[0]->device;
    set->plan.n_keys = n_keys;
    std::vector<KeyRec> recs(n_keys);
    for (uint32_t j = 0; j < n_keys; j++) {
        recs[j] = KeyRec{keys[j]->ic.p, keys[j]->tab.p, keys[j]->ml_ab.p, keys[j]->nPublic, 0};
        set->nPublic.push_back(keys[j]->nPublic);
        set->alpha_h.insert(set->alpha_h.end(), keys[j]->alpha_h, keys[j]->alpha_h + 64);
        set->beta_h.insert(set->beta_h.end(), keys[j]->beta_h, keys[j]->beta_h + 128);
    }
    DeviceGuard g(set->device);
    Stream st;
    set->kc.make(st.s);
    set->recs.alloc(n_keys);
    set->recs.upload(recs.data(), n_keys, st.s);
    HIP_TRY(hipStreamSynchronize(st.s));
    return set.release();
}

// at[i]: where proof i's signals begin; at[n]: the call's total
void set_verify_coop(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, const std::vector<uint64_t> &at, uint64_t n,
                     uint8_t *verdict) {
    zk_vkey_set::Coop &c = set->coop;
    const uint64_t npub = at[n];
    if (!c.st) c.st.reset(new Stream);
    if (c.cap < n) {
        need_hbm("zk_vkey_set_verify", n * (256 + 1 + 4 + 8 + MILLER_LINES * sizeof(Line)) + npub * 32 + 65536);
        c.cap = 0;
        c.dp.alloc(n * 256);
        c.dv.alloc(n);
        c.dkey.alloc(n);
        c.dat.alloc(n);
        c.lines.alloc(n * MILLER_LINES);
        c.cap = n;
    }
    if (c.cap_pub < npub) {
        c.cap_pub = 0;
        c.dpub.alloc(npub);
        c.cap_pub = npub;
    }
    hipStream_t s = c.st->s;
    HIP_TRY(hipMemcpyAsync(c.dp.p, proofs, n * 256, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c.dkey.p, key_of, n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c.dat.p, at.data(), n * 8, hipMemcpyHostToDevice, s));
    if (npub) HIP_TRY(hipMemcpyAsync(c.dpub.p, publics, npub * 32, hipMemcpyHostToDevice, s));
    ZK_LAUNCH(k_set_coop, dim3((uint32_t)n), dim3(VERIFY_THREADS), 0, s, c.dv.p, c.dp.p, c.dpub.p, c.dkey.p, c.dat.p, set->recs.p, set->kc.k.p, c.lines.p,
              curve_b<Fq>(), curve_b<Fq2>(), endo_const<Fq>());
    ZK_LAUNCH_OK("cooperative verification of a key set");
    HIP_TRY(hipMemcpyAsync(verdict, c.dv.p, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    set->plan.last_path = ZK_VERIFY_PATH_COOP;
    set->plan.last_launches = 1;
    set->plan.last_waves_padded = 0;
    set->plan.proofs_coop += n;
}

// The layout of one chunk of the lane path: the proofs of caller positions off .. off + cnt - 1 grouped by key, the keys in
// rising order, a key's proofs in the caller's order, every key's run padded to whole waves.
struct ChunkLayout {
    std::vector<uint64_t> count, slot0, pub0;         // per key: its proofs in the chunk, its first slot, its first signal
    std::vector<uint32_t> present;                    // the keys with proofs in the chunk
    std::vector<WaveRec> waves;
    uint64_t npub = 0, padded = 0;
    explicit ChunkLayout(size_t n_keys) : count(n_keys, 0), slot0(n_keys), pub0(n_keys) {}
    void plan(const uint32_t *key_of, uint64_t cnt, const std::vector<uint32_t> &nPublic) {
        for (uint32_t k : present) count[k] = 0;
        present.clear();
        waves.clear();
        npub = padded = 0;
        for (uint64_t i = 0; i < cnt; i++)
            if (count[key_of[i]]++ == 0) present.push_back(key_of[i]);
        std::sort(present.begin(), present.end());
        for (uint32_t k : present) {
            slot0[k] = (uint64_t)waves.size() * 64;
            pub0[k] = npub;
            for (uint64_t done = 0; done < count[k]; done += 64) {
                const uint32_t live = (uint32_t)(count[k] - done < 64 ? count[k] - done : 64);
                waves.push_back(WaveRec{npub, k, live});
                npub += (uint64_t)live * nPublic[k];
            }
            padded += count[k] % 64 != 0;
        }
    }
};

void set_verify_lanes(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, const std::vector<uint64_t> &at, uint64_t n,
                      uint8_t *verdict, uint64_t chunk) {
    const uint64_t cap = n < chunk ? n : chunk;
    ChunkLayout lay(set->nPublic.size());
    // what the largest chunk needs: at most cap + 63 min(n_keys, cap) slots, whatever n
    uint64_t cap_waves = 0, cap_pub = 0;
    for (uint64_t off = 0; off < n; off += cap) {
        lay.plan(key_of + off, n - off < cap ? n - off : cap, set->nPublic);
        cap_waves = lay.waves.size() > cap_waves ? lay.waves.size() : cap_waves;
        cap_pub = lay.npub > cap_pub ? lay.npub : cap_pub;
    }
    const uint64_t cap_slots = cap_waves * 64;
    need_hbm("zk_vkey_set_verify", cap_slots * (256 + 4 + sizeof(G1Affine) + sizeof(Fq12) + 1) + cap_pub * 32 + cap_waves * sizeof(WaveRec) + 65536);
    Stream st;
    hipStream_t s = st.s;
    DevBuf<uint8_t> dp, dv;
    DevBuf<Fr> dpub;
    DevBuf<uint32_t> dst;
    DevBuf<G1Affine> dx;
    DevBuf<Fq12> df;
    DevBuf<WaveRec> dw;
    dp.alloc(cap_slots * 256);
    dv.alloc(cap_slots);
    dpub.alloc(cap_pub);
    dst.alloc(cap_slots);
    dx.alloc(cap_slots);
    df.alloc(cap_slots);
    dw.alloc(cap_waves);
    std::vector<uint8_t> hp(cap_slots * 256), hpub(cap_pub * 32), hv(cap_slots);
    std::vector<uint64_t> slot_of(cap), filled(set->nPublic.size());
    set->plan.last_path = ZK_VERIFY_PATH_LANES;
    set->plan.last_launches = 0;
    set->plan.last_waves_padded = 0;
    for (uint64_t off = 0; off < n; off += cap) {
        const uint64_t cnt = n - off < cap ? n - off : cap;
        lay.plan(key_of + off, cnt, set->nPublic);
        for (uint32_t k : lay.present) filled[k] = 0;
        for (uint64_t i = 0; i < cnt; i++) {
            const uint32_t k = key_of[off + i];
            const uint64_t pos = filled[k]++, slot = lay.slot0[k] + pos, pb = (uint64_t)set->nPublic[k] * 32;
            slot_of[i] = slot;
            memcpy(hp.data() + slot * 256, proofs + (off + i) * 256, 256);
            if (pb) memcpy(hpub.data() + lay.pub0[k] * 32 + pos * pb, publics + at[off + i] * 32, pb);
        }
        const uint64_t nw = lay.waves.size();
        const dim3 grid((uint32_t)nw), block(64);
        HIP_TRY(hipMemcpyAsync(dp.p, hp.data(), nw * 64 * 256, hipMemcpyHostToDevice, s));
        if (lay.npub) HIP_TRY(hipMemcpyAsync(dpub.p, hpub.data(), lay.npub * 32, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dw.p, lay.waves.data(), nw * sizeof(WaveRec), hipMemcpyHostToDevice, s));
        ZK_LAUNCH(k_set_check, grid, block, 0, s, dst.p, dx.p, dp.p, dpub.p, dw.p, set->recs.p, curve_b<Fq>(), curve_b<Fq2>());
        ZK_LAUNCH(k_set_miller, grid, block, 0, s, df.p, dst.p, dp.p, dx.p, dw.p, set->recs.p, set->kc.k.p);
        ZK_LAUNCH(k_set_final, grid, block, 0, s, dv.p, df.p, dst.p, dw.p, set->kc.k.p);
        ZK_LAUNCH_OK("verification of a key set");
        HIP_TRY(hipMemcpyAsync(hv.data(), dv.p, nw * 64, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint64_t i = 0; i < cnt; i++) verdict[off + i] = hv[slot_of[i]];
        set->plan.last_launches += 3;
        set->plan.last_waves_padded += lay.padded;
        set->plan.proofs_lanes += cnt;
    }
}

void set_verify(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t n, uint8_t *verdict) {
    if (!set) throw std::invalid_argument("null argument");
    if (!n) return;
    if (!proofs || !key_of || !verdict) throw std::invalid_argument("null argument");
    const uint64_t n_keys = set->nPublic.size();
    std::vector<uint64_t> at(n + 1);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (key_of[i] >= n_keys)
            throw std::invalid_argument("zk_vkey_set_verify: key_of[" + std::to_string(i) + "] = " + std::to_string(key_of[i]) + ", the set holds " +
                                        std::to_string(n_keys) + " keys");
        at[i] = total;
        total += set->nPublic[key_of[i]];
    }
    at[n] = total;
    if (publics_bytes != total * 32)
        throw std::invalid_argument("zk_vkey_set_verify: publics_bytes: " + std::to_string(total * 32) + " expected (" + std::to_string(total) +
                                    " signals of 32 bytes), " + std::to_string(publics_bytes) + " given");
    if (total && !publics) throw std::invalid_argument("null argument");
    std::lock_guard<std::mutex> lock(set->mu);
    DeviceGuard g(set->device);
    set_verify_locked(set, proofs, key_of, publics, at, n, verdict);
}

}   // namespace

void zkp::set_verify_locked(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, const std::vector<uint64_t> &at, uint64_t n,
                            uint8_t *verdict) {
    const uint64_t coop_max = verify_coop_max(), chunk = chunk_jobs();
    if (n <= coop_max && n <= COOP_MAX_PROOFS) set_verify_coop(set, proofs, key_of, publics, at, n, verdict);
    else set_verify_lanes(set, proofs, key_of, publics, at, n, verdict, chunk);
}

extern "C" {

int zk_vkey_set_create(zk_vkey_set **out, zk_vkey *const *keys, uint32_t n_keys) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        *out = set_create(keys, n_keys);
    });
}

void zk_vkey_set_destroy(zk_vkey_set *set) {
    if (!set) return;
    int prev = -1;
    const bool had = hipGetDevice(&prev) == hipSuccess;
    (void)hipSetDevice(set->device);
    delete set;
    if (had) (void)hipSetDevice(prev);
}

int zk_vkey_set_verify(zk_vkey_set *set, const uint8_t *proofs, const uint32_t *key_of, const uint8_t *publics, uint64_t publics_bytes, uint64_t n,
                       uint8_t *verdict) {
    return guarded([&] { set_verify(set, proofs, key_of, publics, publics_bytes, n, verdict); });
}

int zk_vkey_set_info(zk_vkey_set *set, zk_vkey_set_plan *plan) {
    return guarded([&] {
        if (!set || !plan) throw std::invalid_argument("null argument");
        const uint32_t size = plan->size && plan->size < sizeof *plan ? plan->size : (uint32_t)sizeof *plan;
        std::lock_guard<std::mutex> lock(set->mu);
        zk_vkey_set_plan p = set->plan;
        p.size = size;
        memcpy(plan, &p, size);
    });
}

}   // extern "C"
