// The checker of r1cs.hip for the library's other units (zkey_verify.hip): the segmented row sum A.x | B.x | C.x for a
// vector x that is already on the checker's device, without a witness check around it.  The checker stays r1cs.hip's; a
// unit that made it (zk_r1cs_create) and shares it with no other thread may call these between its own launches on the
// checker's stream.
#pragma once
#include "hiputil.hpp"

namespace zkp {

struct R1csDev {
    int device;
    hipStream_t stream;                             // everything the checker enqueues goes here
    uint32_t nWires, nPublic, m;
    uint64_t nnz;
    const Fr *rows;                                 // 3m values after r1cs_spmv: A.x, then B.x, then C.x, each value * 2^261 mod r
};
R1csDev r1cs_dev(zk_r1cs *r);
// rows = A.x | B.x | C.x (enqueued on the checker's stream); x: nWires values in standard form on the device.  m = 0: nothing
void r1cs_spmv(zk_r1cs *r, const Fr *x);

}   // namespace zkp
