// k = k1 + k2 lambda (mod r) with 0 < k1, k2 < 2^128: the split of a scalar by BN254's endomorphism with NO signs to carry,
// one function for the host (zk_glv_split) and for every lane of mulvec.hip's kernels.
//
// The lattice {(x, y) : x + y lambda = 0 mod r} has the reduced basis v1 = (A, -B), v2 = (C, A) of scale.hip, A^2 + B C = r
// (and C = A + B).  Over the rationals (k, 0) = x1 v1 + x2 v2 with x1 = k A / r, x2 = k B / r.  They are rounded with the
// truncated reciprocals GA = floor(2^256 A / r), GB = floor(2^256 B / r):
//     a = floor((k GA + 2^255) / 2^256),   b = floor((k GB + 2^255) / 2^256),
// and the result is (k, 0) - a v1 - b v2 + (v2 - v1):
//     k1 = k - a A - b C + (C - A),        k2 = a B - b A + (A + B).
//
// The bound.  k GA / 2^256 = x1 - eta with 0 <= eta < k / 2^256 < r / 2^256 < 1/4, so e1 = x1 - a lies in
// [eta - 1/2, eta + 1/2), a part of [-1/2, 3/4); the same for e2 = x2 - b.  With them
//     k1 = (e1 - 1) A + (e2 + 1) C   lies in   [C/2 - 3A/2, 7C/4),
//     k2 = (1 - e1) B + (1 + e2) A   lies in   (B/4 + A/2, 3B/2 + 7A/4],
// and with A < 2^64, 2^126 < B < C < (4/7) 2^128 both intervals are inside (0, 2^128): k1 > 2^125 - 2^65 > 0,
// k1 < 2^128, k2 > 0, k2 < (6/7) 2^128 + 2^65 < 2^128.  k = 0 gives a = b = 0 and the split (C - A, A + B), whose sum
// (C - A) + (A + B) lambda = v2 - v1 is 0 mod r.  Because both halves are known to lie in [0, 2^128), only the low 128 bits
// of the two expressions are computed.  a <= A + 1 and b <= B + 1 fit 128 bits.
#pragma once
#include "field.hpp"

namespace zk {

struct GlvConsts {
    static constexpr u32 A[4] = {0x94d213e3u, 0x89d32568u, 0, 0};
    static constexpr u32 B[4] = {0x7d4f1128u, 0x8211bbebu, 0xeeb859fcu, 0x6f4d8248u};
    static constexpr u32 C[4] = {0x1221250bu, 0x0be4e154u, 0xeeb859fdu, 0x6f4d8248u};
    static constexpr u32 GA[3] = {0xc7e0b3d7u, 0xd91d232eu, 0x00000002u};                              // floor(2^256 A / r), 66 bits
    static constexpr u32 GB[5] = {0x391eb18du, 0x7a7bd9d4u, 0xa773d2cfu, 0x4ccef014u, 0x00000002u};    // floor(2^256 B / r), 130 bits
};

// the low 128 bits of floor((k g + 2^255) / 2^256) for a 256-bit k and a reciprocal g of N words
template <int N>
ZK_HD void glv_round(u32 out[4], const u32 k[8], const u32 g[N]) {
    u32 t[8 + N];
#pragma unroll
    for (int i = 0; i < 8 + N; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        u32 carry = 0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const u64 s = (u64)k[i] * g[j] + t[i + j] + carry;
            t[i + j] = (u32)s;
            carry = (u32)(s >> 32);
        }
        t[i + N] = carry;
    }
    u32 c = 0;
    t[7] = addc(t[7], 0x80000000u, c);
#pragma unroll
    for (int i = 8; i < 8 + N; i++) t[i] = addc(t[i], 0u, c);
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = i < N ? t[8 + i] : 0u;
}

// acc += sign x y, all mod 2^128
ZK_HD void glv_mul_acc(u32 acc[4], const u32 x[4], const u32 y[4], bool negative) {
    u32 p[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        u32 carry = 0;
#pragma unroll
        for (int j = 0; i + j < 4; j++) {
            const u64 s = (u64)x[i] * y[j] + p[i + j] + carry;
            p[i + j] = (u32)s;
            carry = (u32)(s >> 32);
        }
    }
    u32 c = 0;
    if (negative) {
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = subb(acc[i], p[i], c);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = addc(acc[i], p[i], c);
    }
}

// k: 8 words, little-endian, standard form, below r.  k1, k2: 4 words each.
ZK_HD void glv_split(const u32 k[8], u32 k1[4], u32 k2[4]) {
    u32 A[4], B[4], C[4], ga[3], gb[5];                 // copies: the constants are read with constant indices only
#pragma unroll
    for (int i = 0; i < 4; i++) {
        A[i] = GlvConsts::A[i];
        B[i] = GlvConsts::B[i];
        C[i] = GlvConsts::C[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) ga[i] = GlvConsts::GA[i];
#pragma unroll
    for (int i = 0; i < 5; i++) gb[i] = GlvConsts::GB[i];
    u32 a[4], b[4];
    glv_round<3>(a, k, ga);
    glv_round<5>(b, k, gb);
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) k1[i] = addc(k[i], B[i], c);                     // k + (C - A); C - A = B
    glv_mul_acc(k1, a, A, true);
    glv_mul_acc(k1, b, C, true);
#pragma unroll
    for (int i = 0; i < 4; i++) k2[i] = C[i];                                    // A + B = C
    glv_mul_acc(k2, a, B, false);
    glv_mul_acc(k2, b, A, true);
}

}   // namespace zk
