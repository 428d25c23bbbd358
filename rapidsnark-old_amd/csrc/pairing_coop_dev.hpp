// The device side of the cooperative (latency) path that its translation units share: the workgroup's LDS block, the
// sliced Fq12 operations of wave 0, and the body of a workgroup that verifies one proof.  pairing_coop.hip's kernels take
// the key from their launch arguments, pairing_set.hip's from a record in device memory; both run this code.  The tails of
// the two batch units (verify_batch_dev.hpp) run on the same LDS block and sliced operations.  Everything here has
// internal linkage: each unit that includes it gets its own LDS block and its own copies of the functions.
// The lane map is pairing_coop.hpp's; DESIGN.md section 22 has the division of work and the synchronisation.
#pragma once
#include "hiputil.hpp"
#include "devmem.hpp"
#include "ptcheck.hpp"
#include "pairing.hpp"
#include "paircheck.hpp"
#include "ptengine.hpp"
#include "mulglv.hpp"
#include "pairing_coop.hpp"

namespace {

constexpr uint32_t VERIFY_THREADS = 192, PAIRING_THREADS = 128;

// the Fq12 values wave 0 keeps in LDS: the Miller value, then final_exp's variables under their names there
enum { E_IN, E_F, E_T0, E_T1, E_FX, E_FX2, E_FX3, E_Y0, E_Y2, E_Y3, E_Y4, E_Y6, E_COUNT };

struct alignas(16) CoopLds {
    Fq2 prod[36];                                     // a_i b_j of the product under way
    Fq2 e[E_COUNT][6];                                // [value][power of w]
    G1XYZZ part[64];                                  // vk_x's partial sums
    G1Affine pt[3];                                   // -A, vk_x, C
    uint32_t bad_format, bad_point, have_x;
};
static_assert(sizeof(CoopLds) < 16384, "LDS of a cooperative workgroup");
__shared__ CoopLds L;

__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---------------------------------------------------------------- sliced Fq12, wave 0 only (threadIdx.x < 64)
__device__ __noinline__ void c_mul(int r, int a, int b) {
    const int lane = threadIdx.x;
    if (lane < COOP_LANES_FULL) {
        int i, j;
        coop_pair_full(lane, i, j);
        L.prod[lane] = Fq2::mul(L.e[a][i], L.e[b][j]);
    }
    wsync();
    if (lane < 6) L.e[r][lane] = coop_sum(lane, L.prod, COOP_FULL);
    wsync();
}
// f <- f (s P.y + t P.x w + c w^3)
__device__ __noinline__ void c_line(int f, const Line *l, const G1Affine *P) {
    const int lane = threadIdx.x;
    if (lane < COOP_LANES_LINE) {
        int i, j;
        coop_pair_line(lane, i, j);
        const Fq2 coef = load_el(j == 0 ? &l->s : j == 1 ? &l->t : &l->c);
        const Fq scal = j == 0 ? load_el(&P->y) : j == 1 ? load_el(&P->x) : Fq::one();   // times one: the same reduced element
        Fq2 b;
        f2_mul_fq(b, coef, scal);
        L.prod[6 * i + j] = Fq2::mul(L.e[f][i], b);
    }
    wsync();
    if (lane < 6) L.e[f][lane] = coop_sum(lane, L.prod, COOP_LINE);
    wsync();
}
// the maps that act on each coefficient alone: lane k reads and writes only its own
__device__ __noinline__ void c_frob(int r, int a, const PairConsts *k) {
    const int lane = threadIdx.x;
    if (lane < 6) {
        Fq2 x = f2_conj(L.e[a][lane]);
        if (lane) x = Fq2::mul(x, k->gamma1[lane - 1]);
        L.e[r][lane] = x;
    }
    wsync();
}
__device__ __noinline__ void c_frob2(int r, int a, const PairConsts *k) {
    const int lane = threadIdx.x;
    if (lane < 6) {
        Fq2 x = L.e[a][lane];
        if (lane) f2_mul_fq(x, x, k->gamma2[lane - 1]);
        L.e[r][lane] = x;
    }
    wsync();
}
__device__ __forceinline__ void c_conj(int r, int a) {
    const int lane = threadIdx.x;
    if (lane < 6) {
        const Fq2 x = L.e[a][lane];
        L.e[r][lane] = (lane & 1) ? Fq2::neg(x) : x;
    }
    wsync();
}
__device__ __forceinline__ void c_copy(int r, int a) {
    const int lane = threadIdx.x;
    if (lane < 6) L.e[r][lane] = L.e[a][lane];
    wsync();
}
__device__ __forceinline__ void c_one(int r) {
    const int lane = threadIdx.x;
    if (lane < 6) L.e[r][lane] = lane ? Fq2::zero() : Fq2::one();
    wsync();
}
__device__ __noinline__ void c_inv(int r, int a) {
    if (threadIdx.x == 0) {
        Fq12 x, y;
        Fq2 *xs = reinterpret_cast<Fq2 *>(&x), *ys = reinterpret_cast<Fq2 *>(&y);
        for (int k = 0; k < 6; k++) xs[coop_slot(k)] = L.e[a][k];
        f12_inv(y, x);
        for (int k = 0; k < 6; k++) L.e[r][k] = ys[coop_slot(k)];
    }
    wsync();
}
__device__ __noinline__ void c_pow_x(int r, int a) {  // r != a
    c_copy(r, a);
    for (int i = 61; i >= 0; i--) {
        c_mul(r, r, r);
        if ((BN_X >> i) & 1) c_mul(r, r, a);
    }
}
// E_F <- final_exp(E_IN): pairing.hpp's chain, line for line
__device__ __noinline__ void c_final_exp(const PairConsts *k) {
    c_inv(E_T0, E_IN);
    c_conj(E_T1, E_IN);
    c_mul(E_T0, E_T1, E_T0);
    c_frob2(E_T1, E_T0, k);
    c_mul(E_F, E_T1, E_T0);
    c_pow_x(E_FX, E_F);
    c_pow_x(E_FX2, E_FX);
    c_pow_x(E_FX3, E_FX2);
    c_frob(E_T0, E_F, k);
    c_frob2(E_T1, E_F, k);
    c_mul(E_Y0, E_T0, E_T1);
    c_frob(E_T0, E_T1, k);
    c_mul(E_Y0, E_Y0, E_T0);
    c_frob2(E_Y2, E_FX2, k);
    c_frob(E_T0, E_FX, k);
    c_conj(E_Y3, E_T0);
    c_frob(E_T0, E_FX2, k);
    c_mul(E_T0, E_T0, E_FX);
    c_conj(E_Y4, E_T0);
    c_frob(E_T0, E_FX3, k);
    c_mul(E_T0, E_T0, E_FX3);
    c_conj(E_Y6, E_T0);
    c_conj(E_FX2, E_FX2);                             // y5
    c_conj(E_FX, E_F);                                // y1
    c_mul(E_T0, E_Y6, E_Y6);
    c_mul(E_T0, E_T0, E_Y4);
    c_mul(E_T0, E_T0, E_FX2);
    c_mul(E_T1, E_Y3, E_FX2);
    c_mul(E_T1, E_T1, E_T0);
    c_mul(E_T0, E_T0, E_Y2);
    c_mul(E_T1, E_T1, E_T1);
    c_mul(E_T1, E_T1, E_T0);
    c_mul(E_T1, E_T1, E_T1);
    c_mul(E_T0, E_T1, E_FX);
    c_mul(E_T1, E_T1, E_Y0);
    c_mul(E_T0, E_T0, E_T0);
    c_mul(E_F, E_T0, E_T1);
}
// is value e one; for the one lane that gives the verdict
__device__ __forceinline__ bool c_is_one(int e) {
    bool one = L.e[e][0] == Fq2::one();
    for (int c = 1; c < 6; c++) one = one && L.e[e][c].is_zero();
    return one;
}

// the large pieces as functions of their own: inlined, each kernel would carry several copies of the curve arithmetic
__device__ __noinline__ bool nl_subgroup(const G2Affine &Q, const PairConsts *k) {
    const zkp::PsiConsts pk{k->gamma1[1], k->gamma1[2]};
    return zkp::g2_in_subgroup(Q, pk);
}
__device__ __noinline__ bool nl_on_curve(const G1Affine &P, const Fq &b) { return on_curve(P, b); }
__device__ __noinline__ bool nl_on_curve(const G2Affine &Q, const Fq2 &b) { return on_curve(Q, b); }
__device__ __noinline__ void nl_add(G1XYZZ &a, const G1XYZZ &b) { add(a, b); }
__device__ __noinline__ void nl_mul_glv(G1XYZZ &r, const G1Affine &P, const Fr &k, const Fq &beta) { r = mul_glv(P, k, beta); }
__device__ __noinline__ void nl_to_affine(G1Affine &r, const G1XYZZ &p) { r = g1_to_affine(p); }

// ---------------------------------------------------------------- a workgroup per proof
// vk_x = IC_0 + sum pub_j IC_{j+1} into L.pt[1], by the 64 lanes of one wave
__device__ __forceinline__ void vkx_wave(uint32_t lane, const G1Affine *__restrict__ ic, const Fr *__restrict__ pub, uint32_t nPublic, const Fq &beta) {
    G1XYZZ acc = G1XYZZ::inf();
    for (uint32_t j = lane; j < nPublic; j += 64) {
        G1XYZZ t;
        nl_mul_glv(t, load_pt(ic + 1 + j), load_el(pub + j), beta);
        nl_add(acc, t);
    }
    L.part[lane] = acc;
    for (uint32_t s = 32; s; s >>= 1) {
        wsync();
        if (lane < s) {
            G1XYZZ a = L.part[lane];
            const G1XYZZ b = L.part[lane + s];
            nl_add(a, b);
            L.part[lane] = a;
        }
    }
    if (lane == 0) {
        G1XYZZ a = L.part[0];
        nl_add(a, G1XYZZ::from_affine(load_pt(ic)));
        G1Affine X;
        nl_to_affine(X, a);
        L.pt[1] = X;
        L.have_x = X.is_inf() ? 0u : 1u;
    }
}

// The whole of a workgroup of VERIFY_THREADS lanes that verifies one proof.  verdict: the proof's own byte; pr: its 256
// bytes; pub: its nPublic signals; mine: its MILLER_LINES lines, this workgroup's own; ic, tab (gamma's lines, then
// delta's) and ml_ab: the key's.  Every argument is the same in all lanes.  The kernel does nothing after the call: a
// return here ends the lane, and every wave passes the same barriers before it leaves.
__device__ __forceinline__ void verify_coop_proof(uint8_t *verdict, const uint8_t *__restrict__ pr, const Fr *__restrict__ pub, uint32_t nPublic,
                                                  const G1Affine *__restrict__ ic, const Line *__restrict__ tab, const Fq12 *__restrict__ ml_ab,
                                                  const PairConsts *__restrict__ k, Line *mine, const Fq &b1, const Fq2 &b2, const Fq &beta) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const G2Affine *pB = reinterpret_cast<const G2Affine *>(pr + 64);
    if (tid == 0) L.bad_format = L.bad_point = 0;
    __syncthreads();
    // the format: A, B and C on a lane of a wave each, the signals over all lanes
    bool ok = true;
    if (lane == 0) {
        if (wave == 0) {
            G1Affine A = load_pt(reinterpret_cast<const G1Affine *>(pr));
            ok = !A.is_inf() && nl_on_curve(A, b1);
            if (ok) {
                A.y = Fq::neg(A.y);
                L.pt[0] = A;
            }
        } else if (wave == 1) {
            const G2Affine B = load_pt(pB);
            ok = !B.is_inf() && nl_on_curve(B, b2);
        } else {
            const G1Affine C = load_pt(reinterpret_cast<const G1Affine *>(pr + 192));
            ok = !C.is_inf() && nl_on_curve(C, b1);
            if (ok) L.pt[2] = C;
        }
    }
    for (uint32_t j = tid; j < nPublic; j += VERIFY_THREADS) ok = below_r(load_el(pub + j)) && ok;
    if (!ok) atomicOr(&L.bad_format, 1u);
    __syncthreads();
    if (L.bad_format) {                               // the same in every lane
        if (tid == 0) *verdict = ZK_VERIFY_MALFORMED;
        return;
    }
    // side by side: B's lines, B's subgroup test, vk_x
    if (wave == 0) {
        if (lane == 0) line_table(mine, load_pt(pB), *k);
    } else if (wave == 1) {
        if (lane == 0) {
            if (!nl_subgroup(load_pt(pB), k)) L.bad_point = 1;
        }
    } else {
        vkx_wave(lane, ic, pub, nPublic, beta);
    }
    __syncthreads();
    if (L.bad_point) {
        if (tid == 0) *verdict = ZK_VERIFY_MALFORMED;
        return;
    }
    if (wave) return;                                 // no barrier below
    // wave 0: f = miller(-A, B) miller(vk_x, gamma) miller(C, delta) miller(alpha, beta), then the final exponentiation
    c_one(E_IN);
    if (lane < 6) L.e[E_T0][lane] = load_el(reinterpret_cast<const Fq2 *>(ml_ab) + coop_slot(lane));
    wsync();
    const bool have_x = L.have_x != 0;
    const Line *tg = tab, *td = tab + MILLER_LINES;
    int at = 0;
    auto lines3 = [&]() {
        c_line(E_IN, mine + at, &L.pt[0]);
        if (have_x) c_line(E_IN, tg + at, &L.pt[1]);
        c_line(E_IN, td + at, &L.pt[2]);
        at++;
    };
    for (int s = 0; s < 64; s++) {
        c_mul(E_IN, E_IN, E_IN);
        lines3();
        if (ate_bit(s)) lines3();
    }
    lines3();
    lines3();
    c_mul(E_IN, E_IN, E_T0);
    c_final_exp(k);
    if (lane == 0) *verdict = c_is_one(E_F) ? ZK_VERIFY_OK : ZK_VERIFY_INVALID;
}

}   // namespace
