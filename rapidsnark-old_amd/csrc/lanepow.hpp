// A lane's power of a base from the bits of its index: base^l = the product of base^(2^b) over the set bits b of l, at
// most POW_TAB products and on average half the bits of the largest index.  The host makes the table by squaring, the
// kernels of frscan.hip (beta w^(seg L)), plonkquot.hip (g^l, the points g w_m^l) and plonkopen.hip (z^l) walk it.  Each
// unit keeps its own record around the table and its own form of the words: `conv` is applied to every word the host
// writes (the identity for Montgomery words, plonkquot.hip's w29 for the 29-bit kernels).
//
// The walk itself, `for (b = 0; b < POW_TAB && (l >> b); b++) if ((l >> b) & 1) x = mul(x, load(tab + b))`, stays written
// out in each of the three units: as one function template over the field and its loader (by value, by reference, with a
// lambda or a function as the loader) it changed the register allocation of k_scan_reduce<PLONK>, k_scan_apply<PLONK>,
// k_poly_eval or k_plonk_quotient, whichever form was tried; none of the forms left all of them as they were.
#pragma once
#include "ptengine.hpp"

namespace zkp {

constexpr uint32_t POW_TAB = 32;

// base^lanes, what moves a lane from one of its elements to the next, and base^(2^b)
struct PowTab {
    Fr step;
    Fr tab[POW_TAB];
};

template <class Conv>
inline void fill_pow_tab(Fr tab[POW_TAB], Fr base, Conv conv) {
    for (uint32_t b = 0; b < POW_TAB; b++) {
        tab[b] = conv(base);
        base = Fr::sqr(base);
    }
}

// the record of one base (Montgomery) for a grid of `lanes` lanes
template <class Conv>
inline PowTab pow_tab(Fr base, uint64_t lanes, Conv conv) {
    PowTab k;
    k.step = conv(fr_pow(base, lanes));
    fill_pow_tab(k.tab, base, conv);
    return k;
}

}   // namespace zkp
